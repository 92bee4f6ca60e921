/*
 * gsgpu_jni.c -- JNI shim between org.metagene.genestrip.gpu.GsGpuNative and the C ABI (include/gsgpu.h).
 * Not built in the build container (no JDK / jni.h); tests/test_java_glue_cpu.py syntax-checks it against a minimal
 * stand-in for jni.h (tests/native/jni_stub/jni.h: declarations only).  Build on a host with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include \
 *       -o libgsgpu_jni.so gsgpu_jni.c -L../../genestrip_amd -lgshost -lgsgpu
 * tests/test_gpu_jni.py builds it against the stand-in with a small functional JNIEnv (tests/native/jni_stub/jni_env.c) and drives
 * the file-level entry points (hostMatchFiles / hostMatchRun / hostFilterFiles) on the GPU box.
 */
#include <jni.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gsgpu.h"
#include "gshost.h"

#define JNAME(n) Java_org_metagene_genestrip_gpu_GsGpuNative_##n

static void throw_gs(JNIEnv *env, int rc) {
    char msg[512];
    snprintf(msg, sizeof(msg), "gsgpu error %d (%s): %s", rc, gs_strerror(rc), gs_last_error());
    (*env)->ThrowNew(env, (*env)->FindClass(env, "java/lang/RuntimeException"), msg);
}

static void *addr(JNIEnv *env, jobject buf) { return buf ? (*env)->GetDirectBufferAddress(env, buf) : NULL; }

JNIEXPORT jint JNICALL JNAME(deviceCount)(JNIEnv *env, jclass c) {
    int n = 0;
    gs_device_count(&n);
    return n;
}

JNIEXPORT jlong JNICALL JNAME(dbCreate)(JNIEnv *env, jclass c, jint device, jint k, jlong n, jobject kmers, jobject vidx,
                                        jint nValues, jobject parentVi) {
    gs_db *db = NULL;
    int rc = gs_db_create(&db, device, k, n, (const int64_t *)addr(env, kmers), (const int32_t *)addr(env, vidx), nValues,
                          (const int32_t *)addr(env, parentVi));
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)db;
}

JNIEXPORT void JNICALL JNAME(dbCreateStriped)(JNIEnv *env, jclass c, jlongArray devicesThenHandles, jint k, jlong n, jobject kmers,
                                              jobject vidx, jint nValues, jobject parentVi) {
    jsize ns = (*env)->GetArrayLength(env, devicesThenHandles);
    jlong *h = (*env)->GetLongArrayElements(env, devicesThenHandles, NULL);
    int devices[GS_MAX_STRIPES];
    gs_db *dbs[GS_MAX_STRIPES];
    int rc = (ns < 2 || ns > GS_MAX_STRIPES) ? GS_E_INVALID : GS_OK;
    for (jsize i = 0; i < ns && rc == GS_OK; i++) devices[i] = (int)h[i];
    if (rc == GS_OK)
        rc = gs_db_create_striped(dbs, devices, (int)ns, k, n, (const int64_t *)addr(env, kmers), (const int32_t *)addr(env, vidx),
                                  nValues, (const int32_t *)addr(env, parentVi));
    for (jsize i = 0; i < ns && rc == GS_OK; i++) h[i] = (jlong)(intptr_t)dbs[i];
    (*env)->ReleaseLongArrayElements(env, devicesThenHandles, h, rc == GS_OK ? 0 : JNI_ABORT);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbBuildBegin)(JNIEnv *env, jclass c, jint device, jint k, jint nValues, jobject parentVi,
                                            jboolean lowerCaseBases, jint maxDust, jint stepSize) {
    gs_dbbuild *b = NULL;
    int rc = gs_dbbuild_begin(&b, device, k, nValues, (const int32_t *)addr(env, parentVi), lowerCaseBases ? 1 : 0, maxDust, stepSize);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)b;
}

JNIEXPORT void JNICALL JNAME(dbBuildAdd)(JNIEnv *env, jclass c, jlong builder, jobject bases, jobject offsets, jobject nodeVi,
                                         jlong nRegions, jboolean update) {
    int rc = gs_dbbuild_add((gs_dbbuild *)(intptr_t)builder, (const uint8_t *)addr(env, bases), (const uint64_t *)addr(env, offsets),
                            (const int32_t *)addr(env, nodeVi), nRegions, GS_MEM_HOST, update ? 1 : 0);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbBuildFinish)(JNIEnv *env, jclass c, jlong builder) {
    int64_t n = 0;
    int rc = gs_dbbuild_finish((gs_dbbuild *)(intptr_t)builder, &n);
    if (rc) throw_gs(env, rc);
    return (jlong)n;
}

JNIEXPORT void JNICALL JNAME(dbBuildFetch)(JNIEnv *env, jclass c, jlong builder, jobject kmers, jobject valueIdx) {
    int rc = gs_dbbuild_fetch((gs_dbbuild *)(intptr_t)builder, (int64_t *)addr(env, kmers), (int32_t *)addr(env, valueIdx));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbBuildToDb)(JNIEnv *env, jclass c, jlong builder) {
    gs_db *db = NULL;
    int rc = gs_dbbuild_to_db((gs_dbbuild *)(intptr_t)builder, &db);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)db;
}

JNIEXPORT void JNICALL JNAME(dbBuildDestroy)(JNIEnv *env, jclass c, jlong builder) { gs_dbbuild_destroy((gs_dbbuild *)(intptr_t)builder); }

/* ---- store quality, the gs_dbquality family: DBQualityCountsGoal.handleStore.  The capacities are ByteBuffer.capacity() of the buffer in front of them, handed
 * in by the public wrappers of GsGpuNative: every array is checked against them before the library reads or writes it. ---- */
static void throw_short(JNIEnv *env, const char *what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "gsgpu: buffer too small or missing: %s", what);
    (*env)->ThrowNew(env, (*env)->FindClass(env, "java/lang/IllegalArgumentException"), msg);
}

JNIEXPORT jlong JNICALL JNAME(dbQualityBegin)(JNIEnv *env, jclass c, jlong db, jboolean lowerCaseBases, jint maxDust, jint stepSize) {
    gs_dbquality *q = NULL;
    int rc = gs_dbquality_begin(&q, (gs_db *)(intptr_t)db, lowerCaseBases ? 1 : 0, maxDust, stepSize);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)q;
}

JNIEXPORT void JNICALL JNAME(dbQualitySetRange)(JNIEnv *env, jclass c, jlong quality, jlong lo, jlong hi) {
    int rc = gs_dbquality_set_range((gs_dbquality *)(intptr_t)quality, (uint64_t)lo, (uint64_t)hi);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(dbQualityAdd0)(JNIEnv *env, jclass c, jlong quality, jobject bases, jlong basesCap, jobject offsets,
                                            jlong offsetsCap, jobject leafVi, jlong leafViCap, jlong nRegions) {
    const uint64_t *off = (const uint64_t *)addr(env, offsets);
    if (nRegions < 0 || nRegions > (INT64_MAX >> 4)) return throw_short(env, "nRegions");
    if (nRegions > 0) {
        if (!off || offsetsCap < 8 * (nRegions + 1)) return throw_short(env, "offsets (nRegions + 1 x int64)");
        if (!addr(env, leafVi) || leafViCap < 4 * nRegions) return throw_short(env, "leafVi (nRegions x int32)");
        if (!addr(env, bases) || basesCap < 0 || off[nRegions] > (uint64_t)basesCap) return throw_short(env, "bases (offsets[nRegions] bytes)");
    }
    int rc = gs_dbquality_add((gs_dbquality *)(intptr_t)quality, (const uint8_t *)addr(env, bases), off, (const int32_t *)addr(env, leafVi),
                              nRegions, GS_MEM_HOST);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(dbQualityFinish0)(JNIEnv *env, jclass c, jlong quality, jint nValues, jobject counts, jlong countsCap,
                                               jobject present, jlong presentCap) {
    if (nValues < 0 || !addr(env, counts) || countsCap < 24 * (jlong)nValues) return throw_short(env, "counts (nValues x 3 x int64)");
    if (!addr(env, present) || presentCap < (jlong)nValues) return throw_short(env, "present (nValues bytes)");
    int rc = gs_dbquality_finish((gs_dbquality *)(intptr_t)quality, (int64_t *)addr(env, counts), (uint8_t *)addr(env, present));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(dbQualityDestroy)(JNIEnv *env, jclass c, jlong quality) { gs_dbquality_destroy((gs_dbquality *)(intptr_t)quality); }

/* ---- a finished store updated in batches, the gs_dbupdate family: DBGoal.MyFastaReader as a stream.  Capacities as for the dbQuality natives: every direct
 * buffer is checked against the element counts before the library reads or writes it. ---- */
JNIEXPORT jlong JNICALL JNAME(dbUpdateBegin0)(JNIEnv *env, jclass c, jint device, jint k, jint nValues, jobject parentVi, jlong parentViCap,
                                              jboolean lowerCaseBases, jint maxDust, jint stepSize, jobject kmers, jlong kmersCap, jobject valueIdx,
                                              jlong valueIdxCap, jlong nKmers) {
    gs_dbupdate *u = NULL;
    if (nValues < 0 || !addr(env, parentVi) || parentViCap < 4 * (jlong)nValues) return throw_short(env, "parentVi (nValues x int32)"), 0;
    if (nKmers < 0 || nKmers > (INT64_MAX >> 4)) return throw_short(env, "nKmers"), 0;
    if (nKmers > 0) {
        if (!addr(env, kmers) || kmersCap < 8 * nKmers) return throw_short(env, "kmers (nKmers x int64)"), 0;
        if (!addr(env, valueIdx) || valueIdxCap < 4 * nKmers) return throw_short(env, "valueIdx (nKmers x int32)"), 0;
    }
    int rc = gs_dbupdate_begin(&u, device, k, nValues, (const int32_t *)addr(env, parentVi), lowerCaseBases ? 1 : 0, maxDust, stepSize,
                               (const int64_t *)addr(env, kmers), (const int32_t *)addr(env, valueIdx), nKmers, GS_MEM_HOST);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)u;
}

JNIEXPORT jlong JNICALL JNAME(dbUpdateBeginDb)(JNIEnv *env, jclass c, jlong db, jboolean lowerCaseBases, jint maxDust, jint stepSize) {
    gs_dbupdate *u = NULL;
    int rc = gs_dbupdate_begin_db(&u, (gs_db *)(intptr_t)db, lowerCaseBases ? 1 : 0, maxDust, stepSize);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)u;
}

JNIEXPORT void JNICALL JNAME(dbUpdateAdd0)(JNIEnv *env, jclass c, jlong updater, jobject bases, jlong basesCap, jobject offsets, jlong offsetsCap,
                                           jobject nodeVi, jlong nodeViCap, jlong nRegions) {
    const uint64_t *off = (const uint64_t *)addr(env, offsets);
    if (nRegions < 0 || nRegions > (INT64_MAX >> 4)) return throw_short(env, "nRegions");
    if (nRegions > 0) {
        if (!off || offsetsCap < 8 * (nRegions + 1)) return throw_short(env, "offsets (nRegions + 1 x int64)");
        if (!addr(env, nodeVi) || nodeViCap < 4 * nRegions) return throw_short(env, "nodeVi (nRegions x int32)");
        if (!addr(env, bases) || basesCap < 0 || off[nRegions] > (uint64_t)basesCap) return throw_short(env, "bases (offsets[nRegions] bytes)");
    }
    int rc = gs_dbupdate_add((gs_dbupdate *)(intptr_t)updater, (const uint8_t *)addr(env, bases), off, (const int32_t *)addr(env, nodeVi), nRegions,
                             GS_MEM_HOST);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbUpdateFinish)(JNIEnv *env, jclass c, jlong updater) {
    int64_t moved = 0;
    int rc = gs_dbupdate_finish((gs_dbupdate *)(intptr_t)updater, &moved);
    if (rc) throw_gs(env, rc);
    return (jlong)moved;
}

JNIEXPORT jlong JNICALL JNAME(dbUpdateSize)(JNIEnv *env, jclass c, jlong updater) {
    gs_dbupdate_stats st;
    int rc = gs_dbupdate_get_stats((gs_dbupdate *)(intptr_t)updater, &st);
    if (rc) return throw_gs(env, rc), 0;
    return (jlong)st.n_store;
}

JNIEXPORT void JNICALL JNAME(dbUpdateFetch0)(JNIEnv *env, jclass c, jlong updater, jobject kmers, jlong kmersCap, jobject valueIdx,
                                             jlong valueIdxCap) {
    gs_dbupdate_stats st;
    int rc = gs_dbupdate_get_stats((gs_dbupdate *)(intptr_t)updater, &st);
    if (rc) return throw_gs(env, rc);
    if (st.n_store > 0) {
        if (!addr(env, kmers) || kmersCap < 8 * st.n_store) return throw_short(env, "kmers (dbUpdateSize x int64)");
        if (!addr(env, valueIdx) || valueIdxCap < 4 * st.n_store) return throw_short(env, "valueIdx (dbUpdateSize x int32)");
    }
    rc = gs_dbupdate_fetch((gs_dbupdate *)(intptr_t)updater, (int64_t *)addr(env, kmers), (int32_t *)addr(env, valueIdx));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbUpdateToDb)(JNIEnv *env, jclass c, jlong updater) {
    gs_db *db = NULL;
    int rc = gs_dbupdate_to_db((gs_dbupdate *)(intptr_t)updater, &db);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)db;
}

JNIEXPORT void JNICALL JNAME(dbUpdateDestroy)(JNIEnv *env, jclass c, jlong updater) { gs_dbupdate_destroy((gs_dbupdate *)(intptr_t)updater); }

/* ---- a collection sized before it is built, the gs_dbsize family: FillSizeGoal + FillBloomFilterGoal.  Capacities as for the dbQuality natives: every direct
 * buffer is checked against the element counts before the library reads or writes it. ---- */
JNIEXPORT jlong JNICALL JNAME(dbSizeBegin)(JNIEnv *env, jclass c, jint device, jint k, jint nValues, jboolean lowerCaseBases, jint maxDust,
                                           jint stepSize, jint histBits, jint radixBits, jboolean keepKeys) {
    gs_dbsize *s = NULL;
    int rc = gs_dbsize_begin(&s, device, k, nValues, lowerCaseBases ? 1 : 0, maxDust, stepSize, histBits, radixBits, keepKeys ? 1 : 0);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)s;
}

JNIEXPORT void JNICALL JNAME(dbSizeSetRange)(JNIEnv *env, jclass c, jlong sizer, jlong lo, jlong hi) {
    int rc = gs_dbsize_set_range((gs_dbsize *)(intptr_t)sizer, (uint64_t)lo, (uint64_t)hi);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(dbSizeAdd0)(JNIEnv *env, jclass c, jlong sizer, jobject bases, jlong basesCap, jobject offsets, jlong offsetsCap,
                                         jobject tagVi, jlong tagViCap, jlong nRegions) {
    const uint64_t *off = (const uint64_t *)addr(env, offsets);
    if (nRegions < 0 || nRegions > (INT64_MAX >> 4)) return throw_short(env, "nRegions");
    if (nRegions > 0) {
        if (!off || offsetsCap < 8 * (nRegions + 1)) return throw_short(env, "offsets (nRegions + 1 x int64)");
        if (!addr(env, tagVi) || tagViCap < 4 * nRegions) return throw_short(env, "tagVi (nRegions x int32)");
        if (!addr(env, bases) || basesCap < 0 || off[nRegions] > (uint64_t)basesCap) return throw_short(env, "bases (offsets[nRegions] bytes)");
    }
    int rc = gs_dbsize_add((gs_dbsize *)(intptr_t)sizer, (const uint8_t *)addr(env, bases), off, (const int32_t *)addr(env, tagVi), nRegions,
                           GS_MEM_HOST);
    if (rc) throw_gs(env, rc);
}

/* totals: total, dust, included (3 x int64); perValue: nValues x int64; hist: 2^min(histBits, 2k) x int64 -- the sizes the handle was opened with */
JNIEXPORT void JNICALL JNAME(dbSizeCounts0)(JNIEnv *env, jclass c, jlong sizer, jobject totals, jlong totalsCap, jobject perValue, jlong perValueCap,
                                            jobject hist, jlong histCap) {
    gs_dbsize_totals t;
    gs_dbsize_stats st;
    int rc = gs_dbsize_get_stats((gs_dbsize *)(intptr_t)sizer, &st);
    if (rc) return throw_gs(env, rc);
    if (!addr(env, totals) || totalsCap < 24) return throw_short(env, "totals (3 x int64)");
    if (!addr(env, perValue) || perValueCap < 8 * (jlong)st.n_values) return throw_short(env, "perValue (nValues x int64)");
    if (!addr(env, hist) || histCap < 8 * (jlong)st.hist_bins) return throw_short(env, "hist (2^min(histBits, 2k) x int64)");
    rc = gs_dbsize_counts((gs_dbsize *)(intptr_t)sizer, &t, (int64_t *)addr(env, perValue), (int64_t *)addr(env, hist));
    if (rc) return throw_gs(env, rc);
    memcpy(addr(env, totals), &t, sizeof(t));
}

/* bucketSizes: 2^radixBits x int64 (null for a handle opened with radixBits 0); returns the number of distinct k-mers */
JNIEXPORT jlong JNICALL JNAME(dbSizeDistinct0)(JNIEnv *env, jclass c, jlong sizer, jobject bucketSizes, jlong bucketSizesCap) {
    int64_t n = 0;
    gs_dbsize_stats st;
    int rc = gs_dbsize_get_stats((gs_dbsize *)(intptr_t)sizer, &st);
    if (rc) return throw_gs(env, rc), 0;
    if (st.radix_bits > 0 && (!addr(env, bucketSizes) || bucketSizesCap < ((jlong)8 << st.radix_bits)))
        return throw_short(env, "bucketSizes (2^radixBits x int64)"), 0;
    rc = gs_dbsize_distinct((gs_dbsize *)(intptr_t)sizer, &n, st.radix_bits > 0 ? (int64_t *)addr(env, bucketSizes) : NULL);
    if (rc) return throw_gs(env, rc), 0;
    return (jlong)n;
}

/* hist: 2^min(histBits, 2k) x int64; bounds: room for cap + 1 x int64; returns the number of ranges */
JNIEXPORT jint JNICALL JNAME(dbSizePlan0)(JNIEnv *env, jclass c, jobject hist, jlong histCap, jint histBits, jint k, jlong maxPairs, jobject bounds,
                                          jlong boundsCap, jint cap) {
    int n = 0;
    const int hb = histBits < 2 * k ? histBits : 2 * k;
    if (histBits < 1 || histBits > 12 || k < 1 || k > 31) return throw_short(env, "histBits / k"), 0;
    if (!addr(env, hist) || histCap < ((jlong)8 << hb)) return throw_short(env, "hist (2^min(histBits, 2k) x int64)"), 0;
    if (cap < 1 || !addr(env, bounds) || boundsCap < 8 * ((jlong)cap + 1)) return throw_short(env, "bounds (cap + 1 x int64)"), 0;
    int rc = gs_dbsize_plan((const int64_t *)addr(env, hist), histBits, k, maxPairs, (uint64_t *)addr(env, bounds), cap, &n);
    if (rc) return throw_gs(env, rc), 0;
    return n;
}

JNIEXPORT void JNICALL JNAME(dbSizeDestroy)(JNIEnv *env, jclass c, jlong sizer) { gs_dbsize_destroy((gs_dbsize *)(intptr_t)sizer); }

JNIEXPORT void JNICALL JNAME(dbDestroy)(JNIEnv *env, jclass c, jlong db) { gs_db_destroy((gs_db *)(intptr_t)db); }

JNIEXPORT void JNICALL JNAME(dbSave)(JNIEnv *env, jclass c, jlong db, jstring path) {
    const char *p = (*env)->GetStringUTFChars(env, path, NULL);
    int rc = gs_db_save((gs_db *)(intptr_t)db, p);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(dbLoad)(JNIEnv *env, jclass c, jint device, jstring path) {
    gs_db *db = NULL;
    const char *p = (*env)->GetStringUTFChars(env, path, NULL);
    int rc = gs_db_load(&db, device, p);
    (*env)->ReleaseStringUTFChars(env, path, p);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)db;
}

JNIEXPORT jlong JNICALL JNAME(matchBegin)(JNIEnv *env, jclass c, jlong db, jboolean classify, jboolean countUnique,
                                          jint maxPaths, jint threshold, jdouble taxErr, jdouble classErr, jint maxKmerResCounts) {
    gs_match_cfg cfg = {classify ? 1 : 0, countUnique ? 1 : 0, maxPaths, threshold, taxErr, classErr, 0, maxKmerResCounts};
    gs_run *run = NULL;
    int rc = gs_match_begin(&run, (gs_db *)(intptr_t)db, &cfg);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)run;
}

JNIEXPORT void JNICALL JNAME(matchSubmit)(JNIEnv *env, jclass c, jlong run, jobject seq, jobject offsets, jlong nReads,
                                          jlong firstReadNo, jobject classVi, jobject flags) {
    int rc = gs_match_submit((gs_run *)(intptr_t)run, (const uint8_t *)addr(env, seq), (const uint64_t *)addr(env, offsets),
                             nReads, firstReadNo, GS_MEM_HOST, (int32_t *)addr(env, classVi), (uint8_t *)addr(env, flags));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(matchSubmitAsync)(JNIEnv *env, jclass c, jlong run, jobject seq, jobject offsets, jlong nReads,
                                                jlong firstReadNo, jobject classVi, jobject flags) {
    int64_t ticket = -1;
    int rc = gs_match_submit_async((gs_run *)(intptr_t)run, (const uint8_t *)addr(env, seq), (const uint64_t *)addr(env, offsets),
                                   nReads, firstReadNo, (int32_t *)addr(env, classVi), (uint8_t *)addr(env, flags), &ticket);
    if (rc) throw_gs(env, rc);
    return ticket;
}

JNIEXPORT void JNICALL JNAME(matchWait)(JNIEnv *env, jclass c, jlong run, jlong ticket) {
    int rc = gs_match_wait((gs_run *)(intptr_t)run, ticket);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jlong JNICALL JNAME(matchSubmitText)(JNIEnv *env, jclass c, jlong run, jobject text, jlong nBytes, jlong nLines,
                                               jlong firstReadNo) {
    int64_t ticket = -1;
    int rc = gs_match_submit_text((gs_run *)(intptr_t)run, (const uint8_t *)addr(env, text), nBytes, nLines, GS_MEM_HOST,
                                  firstReadNo, NULL, NULL, &ticket);
    if (rc) throw_gs(env, rc);
    return (jlong)ticket;
}

JNIEXPORT void JNICALL JNAME(matchTextWaitCopy)(JNIEnv *env, jclass c, jlong run, jlong ticket) {
    int rc = gs_match_text_wait_copy((gs_run *)(intptr_t)run, ticket);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchTextStatus)(JNIEnv *env, jclass c, jlong run, jlongArray out) {
    int64_t v[5] = {-1, -1, 0, 0, 0};
    int rc = gs_match_text_status((gs_run *)(intptr_t)run, &v[0], &v[1], &v[2]);
    if (rc) throw_gs(env, rc);
    (*env)->SetLongArrayRegion(env, out, 0, 5, (const jlong *)v);
}

JNIEXPORT void JNICALL JNAME(matchTextClearError)(JNIEnv *env, jclass c, jlong run) {
    int rc = gs_match_text_clear_error((gs_run *)(intptr_t)run);
    if (rc) throw_gs(env, rc);
}

/* page-locked staging memory as a direct ByteBuffer: copies from it run at the full host-to-device rate and
 * asynchronously, copies from ordinary (pageable) direct buffers are staged by the runtime */
JNIEXPORT jobject JNICALL JNAME(pinnedAlloc)(JNIEnv *env, jclass c, jlong bytes) {
    void *p = NULL;
    int rc = gs_pinned_alloc(&p, (size_t)bytes);
    if (rc) {
        throw_gs(env, rc);
        return NULL;
    }
    return (*env)->NewDirectByteBuffer(env, p, bytes);
}

JNIEXPORT void JNICALL JNAME(pinnedFree)(JNIEnv *env, jclass c, jobject buf) {
    int rc = gs_pinned_free(addr(env, buf));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchSegments)(JNIEnv *env, jclass c, jlong run, jobject seq, jobject offsets, jlong nReads,
                                            jobject segOff) {
    int rc = gs_match_segments((gs_run *)(intptr_t)run, (const uint8_t *)addr(env, seq), (const uint64_t *)addr(env, offsets),
                               nReads, GS_MEM_HOST, (uint64_t *)addr(env, segOff));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchSegmentsFetch)(JNIEnv *env, jclass c, jlong run, jobject codes, jobject starts) {
    int rc = gs_match_segments_fetch((gs_run *)(intptr_t)run, (int32_t *)addr(env, codes), (int32_t *)addr(env, starts));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchMaxContigReads)(JNIEnv *env, jclass c, jlong run, jobject readNo) {
    int rc = gs_match_max_contig_reads((gs_run *)(intptr_t)run, (int64_t *)addr(env, readNo));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchMaxCounts)(JNIEnv *env, jclass c, jlong run, jobject out) {
    int rc = gs_match_max_counts((gs_run *)(intptr_t)run, (int16_t *)addr(env, out));
    if (rc) throw_gs(env, rc);
}

/* the runs of this JVM (one per GPU) into a global state held by each (RCCL between devices) */
JNIEXPORT void JNICALL JNAME(matchMerge)(JNIEnv *env, jclass c, jlongArray runs) {
    jsize n = (*env)->GetArrayLength(env, runs);
    jlong *h = (*env)->GetLongArrayElements(env, runs, NULL);
    gs_run *r[64];
    int rc = n > 64 ? GS_E_INVALID : GS_OK;
    for (jsize i = 0; i < n && rc == GS_OK; i++) r[i] = (gs_run *)(intptr_t)h[i];
    if (rc == GS_OK) rc = gs_match_merge(r, (int)n);
    (*env)->ReleaseLongArrayElements(env, runs, h, JNI_ABORT);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchFinish)(JNIEnv *env, jclass c, jlong run, jobject table, jobject dtable) {
    int rc = gs_match_finish((gs_run *)(intptr_t)run, (int64_t *)addr(env, table), (double *)addr(env, dtable));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchReset)(JNIEnv *env, jclass c, jlong run) {
    int rc = gs_match_reset((gs_run *)(intptr_t)run);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(matchDestroy)(JNIEnv *env, jclass c, jlong run) { gs_match_destroy((gs_run *)(intptr_t)run); }

JNIEXPORT jlong JNICALL JNAME(bloomBuild)(JNIEnv *env, jclass c, jint device, jobject kmers, jlong nKmers, jlong expectedInsertions,
                                          jdouble fpp) {
    gs_bloom *b = NULL;
    int rc = gs_bloom_build(&b, device, GS_BLOOM_XOR, (const int64_t *)addr(env, kmers), nKmers, GS_MEM_HOST, expectedInsertions, fpp);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)b;
}

JNIEXPORT jlong JNICALL JNAME(bloomCreate)(JNIEnv *env, jclass c, jint device, jint kind, jlong bits, jint nHashes,
                                           jlongArray factors, jobject words, jlong nWords) {
    gs_bloom *b = NULL;
    jlong *f = (*env)->GetLongArrayElements(env, factors, NULL);
    int rc = gs_bloom_create(&b, device, kind, bits, nHashes, (const int64_t *)f, (const uint64_t *)addr(env, words), nWords);
    (*env)->ReleaseLongArrayElements(env, factors, f, JNI_ABORT);
    if (rc) throw_gs(env, rc);
    return (jlong)(intptr_t)b;
}

JNIEXPORT void JNICALL JNAME(bloomDestroy)(JNIEnv *env, jclass c, jlong b) { gs_bloom_destroy((gs_bloom *)(intptr_t)b); }

JNIEXPORT void JNICALL JNAME(filterSubmit)(JNIEnv *env, jclass c, jlong b, jint k, jint minPos, jdouble ratio, jobject seq,
                                           jobject offsets, jlong nReads, jobject accept) {
    int rc = gs_filter_submit((gs_bloom *)(intptr_t)b, k, minPos, ratio, (const uint8_t *)addr(env, seq),
                              (const uint64_t *)addr(env, offsets), nReads, GS_MEM_HOST, (uint8_t *)addr(env, accept), 0);
    if (rc) throw_gs(env, rc);
}

/* ---------------------------------------------------------------------------------------------------
 * The file-level entry points of include/gshost.h: what runMatcher / runFilter call when every resource of the
 * StreamingResourceStream is a local file (FastqKMerMatcher.java:181-235, FastqBloomFilter.java:80-89).  The whole pipeline --
 * file, (device) gunzip, record scan, kernels, per-read outputs (gathered and compressed on the device) -- then runs below the
 * JVM: 11-19 Gbp/s instead of the parser thread's 0.2-0.7.
 * ------------------------------------------------------------------------------------------------- */
static void throw_host(JNIEnv *env, int rc) {
    char msg[640];
    const char *h = gs_host_last_error();
    /* a call stopped on request (GS_E_CANCELLED): the message starts with "cancelled" -- the reference's FastqReaderInterruptedException
     * has no constructor that takes a message, which ThrowNew needs; the Java callers turn this one into it */
    if (rc == GS_E_CANCELLED)
        snprintf(msg, sizeof(msg), "cancelled: gsgpu status %d", rc);
    else
        snprintf(msg, sizeof(msg), "gsgpu error %d (%s): %s", rc, gs_strerror(rc), (h && h[0]) ? h : gs_last_error());
    (*env)->ThrowNew(env, (*env)->FindClass(env, "java/lang/RuntimeException"), msg);
}

/* a Java String[] as a C array of UTF-8 strings (NULL elements stay NULL); released with free_strings */
typedef struct {
    jsize n;
    const char **c;
    jstring *j;
} StrArray;

static int get_strings(JNIEnv *env, jobjectArray a, StrArray *out) {
    out->n = a ? (*env)->GetArrayLength(env, a) : 0;
    out->c = (const char **)calloc((size_t)out->n + 1, sizeof(char *));
    out->j = (jstring *)calloc((size_t)out->n + 1, sizeof(jstring));
    if (!out->c || !out->j) return GS_E_NOMEM;
    for (jsize i = 0; i < out->n; i++) {
        out->j[i] = (jstring)(*env)->GetObjectArrayElement(env, a, i);
        out->c[i] = out->j[i] ? (*env)->GetStringUTFChars(env, out->j[i], NULL) : NULL;
    }
    return GS_OK;
}

static void free_strings(JNIEnv *env, StrArray *s) {
    for (jsize i = 0; i < s->n; i++) {
        if (s->j && s->j[i]) {
            if (s->c && s->c[i]) (*env)->ReleaseStringUTFChars(env, s->j[i], s->c[i]);
            (*env)->DeleteLocalRef(env, s->j[i]);
        }
    }
    free((void *)s->c);
    free(s->j);
}

static void put_totals(JNIEnv *env, jlongArray totals, const gs_host_totals *t) {
    if (!totals) return;
    const jlong v[4] = {t->reads, t->kmers, t->bps, t->filtered_reads};
    (*env)->SetLongArrayRegion(env, totals, 0, 4, v);
}

static void fill_opts(gs_host_match_opts *o, const char *flt, const char *kr, jboolean writeAll, const StrArray *tax, jboolean withProbs, void *desc, jint stride) {
    memset(o, 0, sizeof(*o));
    o->filtered_path = flt;
    o->kraken_out_path = kr;
    o->write_all = writeAll ? 1 : 0;
    o->taxids = tax->n ? tax->c : NULL;
    o->with_probs = withProbs ? 1 : 0;
    o->max_contig_desc = (uint8_t *)desc;
    o->max_contig_desc_stride = stride;
}

/* gs_host_match_files: one call = one runMatcher over local files with a run of its own; totals = {reads, kmers, bps, filtered reads} */
JNIEXPORT void JNICALL JNAME(hostMatchFiles)(JNIEnv *env, jclass c, jlong db, jboolean classify, jboolean countUnique, jint maxPaths, jint threshold,
                                             jdouble taxErr, jdouble classErr, jint maxKmerResCounts, jobjectArray paths, jstring filteredPath,
                                             jstring krakenOutPath, jboolean writeAll, jobjectArray taxids, jboolean withProbs, jobject table,
                                             jobject dtable, jobject maxContigDesc, jint descStride, jlongArray totals) {
    gs_match_cfg cfg = {classify ? 1 : 0, countUnique ? 1 : 0, maxPaths, threshold, taxErr, classErr, 0, maxKmerResCounts};
    StrArray p = {0, NULL, NULL}, tax = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    if (!rc) rc = get_strings(env, taxids, &tax);
    const char *flt = filteredPath ? (*env)->GetStringUTFChars(env, filteredPath, NULL) : NULL;
    const char *kr = krakenOutPath ? (*env)->GetStringUTFChars(env, krakenOutPath, NULL) : NULL;
    gs_host_totals t;
    memset(&t, 0, sizeof(t));
    if (!rc) {
        gs_host_match_opts o;
        fill_opts(&o, flt, kr, writeAll, &tax, withProbs, addr(env, maxContigDesc), descStride);
        rc = gs_host_match_files((gs_db *)(intptr_t)db, &cfg, p.c, (int)p.n, &o, (int64_t *)addr(env, table), (double *)addr(env, dtable), &t);
    }
    if (flt) (*env)->ReleaseStringUTFChars(env, filteredPath, flt);
    if (kr) (*env)->ReleaseStringUTFChars(env, krakenOutPath, kr);
    free_strings(env, &p);
    free_strings(env, &tax);
    if (!rc || rc == GS_E_CANCELLED) put_totals(env, totals, &t);  /* (a stopped call has filled them: in front of the throw) */
    if (rc) throw_host(env, rc);
}

/* gs_host_match_run: the same into the matcher's own run (matchReset before, matchFinish after) */
JNIEXPORT void JNICALL JNAME(hostMatchRun)(JNIEnv *env, jclass c, jlong run, jlong db, jobjectArray paths, jstring filteredPath, jstring krakenOutPath,
                                           jboolean writeAll, jobjectArray taxids, jboolean withProbs, jobject maxContigDesc, jint descStride,
                                           jlongArray totals) {
    StrArray p = {0, NULL, NULL}, tax = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    if (!rc) rc = get_strings(env, taxids, &tax);
    const char *flt = filteredPath ? (*env)->GetStringUTFChars(env, filteredPath, NULL) : NULL;
    const char *kr = krakenOutPath ? (*env)->GetStringUTFChars(env, krakenOutPath, NULL) : NULL;
    gs_host_totals t;
    memset(&t, 0, sizeof(t));
    if (!rc) {
        gs_host_match_opts o;
        fill_opts(&o, flt, kr, writeAll, &tax, withProbs, addr(env, maxContigDesc), descStride);
        rc = gs_host_match_run((gs_run *)(intptr_t)run, (gs_db *)(intptr_t)db, p.c, (int)p.n, &o, &t);
    }
    if (flt) (*env)->ReleaseStringUTFChars(env, filteredPath, flt);
    if (kr) (*env)->ReleaseStringUTFChars(env, krakenOutPath, kr);
    free_strings(env, &p);
    free_strings(env, &tax);
    if (!rc || rc == GS_E_CANCELLED) put_totals(env, totals, &t);  /* (a stopped call has filled them: in front of the throw) */
    if (rc) throw_host(env, rc);
}

/* gs_host_match_into: some of the files of a sample into a run that is merged with others (matchMerge) before matchFinish */
JNIEXPORT void JNICALL JNAME(hostMatchInto)(JNIEnv *env, jclass c, jlong run, jlong db, jobjectArray paths, jintArray fileIndex, jlongArray readsOfFile,
                                            jlongArray totals) {
    StrArray p = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    jint *idx = fileIndex ? (*env)->GetIntArrayElements(env, fileIndex, NULL) : NULL;
    jlong *rof = readsOfFile ? (*env)->GetLongArrayElements(env, readsOfFile, NULL) : NULL;
    gs_host_totals t;
    memset(&t, 0, sizeof(t));
    if (!rc && (!idx || !rof || (*env)->GetArrayLength(env, fileIndex) < p.n || (*env)->GetArrayLength(env, readsOfFile) < p.n)) rc = GS_E_INVALID;
    if (!rc) rc = gs_host_match_into((gs_run *)(intptr_t)run, (gs_db *)(intptr_t)db, p.c, (int)p.n, (const int32_t *)idx, (int64_t *)rof, &t);
    if (idx) (*env)->ReleaseIntArrayElements(env, fileIndex, idx, JNI_ABORT);
    /* (a stopped call has filled the per-file prefixes: the caller needs them to convert the max-contig read numbers) */
    if (rof) (*env)->ReleaseLongArrayElements(env, readsOfFile, rof, rc && rc != GS_E_CANCELLED ? JNI_ABORT : 0);
    free_strings(env, &p);
    if (!rc || rc == GS_E_CANCELLED) put_totals(env, totals, &t);  /* (a stopped call has filled them: in front of the throw) */
    if (rc) throw_host(env, rc);
}

/* gs_host_filter_files: one call = one runFilter over local files */
JNIEXPORT void JNICALL JNAME(hostFilterFiles)(JNIEnv *env, jclass c, jlong bloom, jint k, jint minPosCount, jdouble positiveRatio, jobjectArray paths,
                                              jstring filteredPath, jstring restPath, jboolean withProbs, jlongArray totals) {
    StrArray p = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    const char *flt = filteredPath ? (*env)->GetStringUTFChars(env, filteredPath, NULL) : NULL;
    const char *rest = restPath ? (*env)->GetStringUTFChars(env, restPath, NULL) : NULL;
    gs_host_totals t;
    memset(&t, 0, sizeof(t));
    if (!rc) rc = gs_host_filter_files((gs_bloom *)(intptr_t)bloom, k, minPosCount, positiveRatio, p.c, (int)p.n, flt, rest, withProbs ? 1 : 0, &t);
    if (flt) (*env)->ReleaseStringUTFChars(env, filteredPath, flt);
    if (rest) (*env)->ReleaseStringUTFChars(env, restPath, rest);
    free_strings(env, &p);
    if (!rc || rc == GS_E_CANCELLED) put_totals(env, totals, &t);  /* (a stopped call has filled them: in front of the throw) */
    if (rc) throw_host(env, rc);
}

/* gs_host_extract_files: the extract goal over local files (ExtractGoal.doMakeThis with writeFilteredFastq); totals[3] = reads written */
JNIEXPORT void JNICALL JNAME(hostExtractFiles)(JNIEnv *env, jclass c, jint device, jstring key, jint k, jobjectArray paths, jstring outPath,
                                               jlongArray totals) {
    StrArray p = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    const char *ky = key ? (*env)->GetStringUTFChars(env, key, NULL) : NULL;
    const char *out = outPath ? (*env)->GetStringUTFChars(env, outPath, NULL) : NULL;
    gs_host_totals t;
    memset(&t, 0, sizeof(t));
    if (!rc) rc = gs_host_extract_files(device, ky, k, p.c, (int)p.n, out, &t);
    if (ky) (*env)->ReleaseStringUTFChars(env, key, ky);
    if (out) (*env)->ReleaseStringUTFChars(env, outPath, out);
    free_strings(env, &p);
    if (!rc || rc == GS_E_CANCELLED) put_totals(env, totals, &t);  /* (a stopped call has filled them: in front of the throw) */
    if (rc) throw_host(env, rc);
}

/* gs_host_fasta2fastq: Fasta2FastqGoal.makeFile over local files; returns the records written */
JNIEXPORT jlong JNICALL JNAME(hostFasta2Fastq)(JNIEnv *env, jclass c, jint device, jobjectArray paths, jstring outPath) {
    StrArray p = {0, NULL, NULL};
    int rc = get_strings(env, paths, &p);
    const char *out = outPath ? (*env)->GetStringUTFChars(env, outPath, NULL) : NULL;
    int64_t n = 0;
    if (!rc) rc = gs_host_fasta2fastq(device, p.c, (int)p.n, out, &n);
    if (out) (*env)->ReleaseStringUTFChars(env, outPath, out);
    free_strings(env, &p);
    if (rc) throw_host(env, rc);
    return (jlong)n;
}

/* gs_host_last_error */
JNIEXPORT jstring JNICALL JNAME(hostLastError)(JNIEnv *env, jclass c) { return (*env)->NewStringUTF(env, gs_host_last_error()); }

/* ---- progress and cancellation (include/gshost.h, gs_host_control_*).  The stand-in jni.h of the test-suite has no method-call
 * functions, so nothing calls back into Java: the handle is made without a callback, a Java thread polls hostControlSnapshot and
 * calls hostControlCancel.  hostControlAttach is per thread: the thread that attaches makes the file-level call. ---- */
JNIEXPORT jlong JNICALL JNAME(hostControlCreate)(JNIEnv *env, jclass c) {
    gs_host_control *h = NULL;
    int rc = gs_host_control_create(&h, NULL, NULL, 0);
    if (rc) throw_host(env, rc);
    return (jlong)(intptr_t)h;
}

JNIEXPORT void JNICALL JNAME(hostControlDestroy)(JNIEnv *env, jclass c, jlong control) {
    int rc = gs_host_control_destroy((gs_host_control *)(intptr_t)control);
    if (rc) throw_host(env, rc);
}

JNIEXPORT void JNICALL JNAME(hostControlCancel)(JNIEnv *env, jclass c, jlong control) {
    int rc = gs_host_control_cancel((gs_host_control *)(intptr_t)control);
    if (rc) throw_host(env, rc);
}

/* control = 0 detaches */
JNIEXPORT void JNICALL JNAME(hostControlAttach)(JNIEnv *env, jclass c, jlong control) {
    int rc = gs_host_control_attach((gs_host_control *)(intptr_t)control);
    if (rc) throw_host(env, rc);
}

/* out[13]: file, n_files, file_done, files_done, file_bytes_done, file_bytes_total, file_reads, total_bytes_done, total_bytes_total,
 * total_reads, the file's and the call's time in milliseconds, cancelled (0 / 1) */
JNIEXPORT void JNICALL JNAME(hostControlSnapshot)(JNIEnv *env, jclass c, jlong control, jlongArray out) {
    gs_host_progress p;
    int32_t cancelled = 0;
    int rc = gs_host_control_snapshot((gs_host_control *)(intptr_t)control, &p, &cancelled);
    if (!rc && (!out || (*env)->GetArrayLength(env, out) < 13)) rc = GS_E_INVALID;
    if (rc) {
        throw_host(env, rc);
        return;
    }
    const jlong v[13] = {p.file, p.n_files, p.file_done, p.files_done, p.file_bytes_done, p.file_bytes_total, p.file_reads, p.total_bytes_done,
                         p.total_bytes_total, p.total_reads, (jlong)(p.seconds_file * 1e3), (jlong)(p.seconds_total * 1e3), cancelled};
    (*env)->SetLongArrayRegion(env, out, 0, 13, v);
}

/* gs_host_release_pools */
JNIEXPORT void JNICALL JNAME(hostReleasePools)(JNIEnv *env, jclass c) {
    int rc = gs_host_release_pools();
    if (rc) throw_host(env, rc);
}
