/*
 * gsgpu_jni.c -- JNI shim between org.metagene.genestrip.gpu.GsGpuNative and the C ABI (include/gsgpu.h).
 * Not built in the build container (no JDK / jni.h); tests/test_java_glue_cpu.py syntax-checks it against a minimal
 * stand-in for jni.h (tests/native/jni_stub/jni.h: declarations only).  Build on a host with a JDK:
 *   gcc -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include \
 *       -o libgsgpu_jni.so gsgpu_jni.c -L../../genestrip_amd -lgshost -lgsgpu
 * tests/test_gpu_jni.py builds it against the stand-in with a small functional JNIEnv (tests/native/jni_stub/jni_env.c) and drives
 * the file-level entry points (hostMatchFiles / hostMatchRun / hostFilterFiles) on the GPU box; tests/test_gpu_jni_dbchain.py does the same
 * for the natives of the database-construction chain at the end of this file.
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

/* ---------------------------------------------------------------------------------------------------
 * The database-construction chain: gs_genomes_*, gs_accmap_*, gs_taxtree_*, gs_asmsum_* and their file-level calls.
 * Arguments in C order; every direct buffer is followed by its capacity in ELEMENTS of its type (keys32, text, pools: bytes), and a
 * call that needs more is refused with IllegalArgumentException before the library sees it.  The C ABI does not say how many
 * elements a fetch writes -- the caller knows from finish -- so a handle of these four families travels as a small record of the
 * shim's own: the library's handle and the counts its calls have reported (JGenomes, JAccmap, JAsmsum, JTaxtree).  Such a long is
 * good for the natives of its family, for accmapLookupGenomes and for hostGenomeFilesInto; the destroy native frees both.
 * No upcalls; int[] / long[] outputs are written through the array's elements.
 * ------------------------------------------------------------------------------------------------- */
typedef struct {
    gs_genomes *g;
    int64_t n_records, header_bytes;
} JGenomes;
typedef struct {
    gs_accmap *am;
    int64_t n_entries; /* -1 in front of finish */
    int32_t n_nodes;
} JAccmap;
typedef struct {
    gs_asmsum *as;
    int64_t n_picked; /* -1 in front of finish */
} JAsmsum;
typedef struct {
    gs_taxtree *t;
    int64_t n_nodes, n_reached; /* -1 in front of finish */
} JTaxtree;

#define JG(h) ((JGenomes *)(intptr_t)(h))
#define JA(h) ((JAccmap *)(intptr_t)(h))
#define JS(h) ((JAsmsum *)(intptr_t)(h))
#define JT(h) ((JTaxtree *)(intptr_t)(h))

/* 1 (and the exception is pending): buf cannot hold `need` elements */
static int too_short(JNIEnv *env, jobject buf, jlong cap, int64_t need, const char *what) {
    if (need < 0 || cap < need || (need > 0 && !addr(env, buf))) {
        throw_short(env, what);
        return 1;
    }
    return 0;
}

static int no_handle(JNIEnv *env, const void *h) {
    if (!h) throw_short(env, "handle is 0");
    return !h;
}

/* long[] out of at least n elements <- v; 1 (and the exception is pending) if it is shorter */
static int put_longs(JNIEnv *env, jlongArray out, const int64_t *v, jsize n, const char *what) {
    if (!out || (*env)->GetArrayLength(env, out) < n) {
        throw_short(env, what);
        return 1;
    }
    (*env)->SetLongArrayRegion(env, out, 0, n, (const jlong *)v);
    return 0;
}

static int longs_short(JNIEnv *env, jlongArray out, jsize n, const char *what) {
    if (!out || (*env)->GetArrayLength(env, out) < n) {
        throw_short(env, what);
        return 1;
    }
    return 0;
}

/* ---- gs_genomes ---- */
JNIEXPORT jlong JNICALL JNAME(genomesCreate)(JNIEnv *env, jclass c, jint device) {
    JGenomes *j = (JGenomes *)calloc(1, sizeof(JGenomes));
    int rc = j ? gs_genomes_create(&j->g, device) : GS_E_NOMEM;
    if (rc) {
        free(j);
        return throw_gs(env, rc), 0;
    }
    return (jlong)(intptr_t)j;
}

/* out[4]: n_records, consumed_bytes, header_bytes, max_line_bytes */
JNIEXPORT void JNICALL JNAME(genomesScan)(JNIEnv *env, jclass c, jlong genomes, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray out) {
    int64_t v[4] = {0, 0, 0, 0};
    if (no_handle(env, JG(genomes)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, out, 4, "out (4 x long)")) return;
    JG(genomes)->n_records = JG(genomes)->header_bytes = 0;
    int rc = gs_genomes_scan(JG(genomes)->g, (const uint8_t *)addr(env, text), nBytes, GS_MEM_HOST, last ? 1 : 0, &v[0], &v[1], &v[2], &v[3]);
    if (rc) return throw_gs(env, rc);
    JG(genomes)->n_records = v[0];
    JG(genomes)->header_bytes = v[2];
    put_longs(env, out, v, 4, "out (4 x long)");
}

JNIEXPORT void JNICALL JNAME(genomesHeaders)(JNIEnv *env, jclass c, jlong genomes, jobject headers, jlong headersCap, jobject headerOff, jlong headerOffCap) {
    if (no_handle(env, JG(genomes)) || too_short(env, headers, headersCap, JG(genomes)->header_bytes, "headers (header_bytes of the scan)") ||
        too_short(env, headerOff, headerOffCap, JG(genomes)->n_records + 1, "headerOff (n_records + 1 x int64)"))
        return;
    int rc = gs_genomes_headers(JG(genomes)->g, (uint8_t *)addr(env, headers), (uint64_t *)addr(env, headerOff));
    if (rc) throw_gs(env, rc);
}

/* keep: null = every record; out[2]: n_regions, n_bases */
JNIEXPORT void JNICALL JNAME(genomesGather)(JNIEnv *env, jclass c, jlong genomes, jobject keep, jlong keepCap, jlongArray out) {
    int64_t v[2] = {0, 0};
    if (no_handle(env, JG(genomes)) || (keep && too_short(env, keep, keepCap, JG(genomes)->n_records, "keep (n_records bytes)")) ||
        longs_short(env, out, 2, "out (2 x long)"))
        return;
    int rc = gs_genomes_gather(JG(genomes)->g, (const uint8_t *)addr(env, keep), &v[0], &v[1]);
    if (rc) return throw_gs(env, rc);
    put_longs(env, out, v, 2, "out (2 x long)");
}

/* out[2]: the DEVICE addresses of seq and off of the last gather */
JNIEXPORT void JNICALL JNAME(genomesRegions)(JNIEnv *env, jclass c, jlong genomes, jlongArray out) {
    const uint8_t *seq = NULL;
    const uint64_t *off = NULL;
    if (no_handle(env, JG(genomes)) || longs_short(env, out, 2, "out (2 x long)")) return;
    int rc = gs_genomes_regions(JG(genomes)->g, &seq, &off);
    if (rc) return throw_gs(env, rc);
    const int64_t v[2] = {(int64_t)(intptr_t)seq, (int64_t)(intptr_t)off};
    put_longs(env, out, v, 2, "out (2 x long)");
}

JNIEXPORT void JNICALL JNAME(genomesDestroy)(JNIEnv *env, jclass c, jlong genomes) {
    if (!JG(genomes)) return;
    gs_genomes_destroy(JG(genomes)->g);
    free(JG(genomes));
}

/* ---- gs_accmap ---- */
/* cats / stats / known must stay alive for the call that uses *cfg; 0, or an exception is pending */
static int accmap_cfg(JNIEnv *env, gs_accmap_cfg *cfg, jboolean dna, jboolean rna, jboolean mrna, const StrArray *cats, const StrArray *stats, jobject known,
                      jlong knownCap, jint nNodes, jlong reserve) {
    if (too_short(env, known, knownCap, nNodes, "knownTaxids (nNodes x int32)")) return 1;
    memset(cfg, 0, sizeof(*cfg));
    cfg->dna = dna ? 1 : 0;
    cfg->rna = rna ? 1 : 0;
    cfg->mrna = mrna ? 1 : 0;
    cfg->n_categories = (int32_t)cats->n;
    cfg->n_statuses = (int32_t)stats->n;
    cfg->n_nodes = nNodes;
    cfg->categories = cats->c;
    cfg->statuses = stats->c;
    cfg->known_taxids = (const int32_t *)addr(env, known);
    cfg->reserve_entries = reserve;
    return 0;
}

JNIEXPORT jlong JNICALL JNAME(accmapCreate)(JNIEnv *env, jclass c, jint device, jboolean dna, jboolean rna, jboolean mrna, jobjectArray categories,
                                            jobjectArray statuses, jobject knownTaxids, jlong knownTaxidsCap, jint nNodes, jlong reserveEntries) {
    StrArray cats = {0, NULL, NULL}, stats = {0, NULL, NULL};
    gs_accmap_cfg cfg;
    JAccmap *j = NULL;
    int rc = get_strings(env, categories, &cats);
    if (!rc) rc = get_strings(env, statuses, &stats);
    int thrown = 0;
    if (!rc && !(thrown = accmap_cfg(env, &cfg, dna, rna, mrna, &cats, &stats, knownTaxids, knownTaxidsCap, nNodes, reserveEntries))) {
        j = (JAccmap *)calloc(1, sizeof(JAccmap));
        rc = j ? gs_accmap_create(&j->am, device, &cfg) : GS_E_NOMEM;
        if (!rc) {
            j->n_entries = -1;
            j->n_nodes = nNodes;
        }
    }
    free_strings(env, &cats);
    free_strings(env, &stats);
    if (rc) {
        free(j);
        j = NULL;
        if (!thrown) throw_gs(env, rc);
    }
    return (jlong)(intptr_t)j;
}

JNIEXPORT void JNICALL JNAME(accmapSubmit)(JNIEnv *env, jclass c, jlong accmap, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray report) {
    int64_t r[8] = {0};
    if (no_handle(env, JA(accmap)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, report, 8, "report (8 x long)")) return;
    int rc = gs_accmap_submit(JA(accmap)->am, (const uint8_t *)addr(env, text), nBytes, GS_MEM_HOST, last ? 1 : 0, r);
    if (rc) return throw_gs(env, rc);
    put_longs(env, report, r, 8, "report (8 x long)");
}

JNIEXPORT void JNICALL JNAME(accmapAppend)(JNIEnv *env, jclass c, jlong accmap, jobject keys32, jlong keys32Cap, jobject nodes, jlong nodesCap, jlong n,
                                           jlong nPassing) {
    if (no_handle(env, JA(accmap))) return;
    if (n < 0 || n > (INT64_MAX >> 6)) return throw_short(env, "n");
    if (too_short(env, keys32, keys32Cap, 32 * n, "keys32 (n x 32 bytes)") || too_short(env, nodes, nodesCap, n, "nodes (n x int32)")) return;
    int rc = gs_accmap_append(JA(accmap)->am, (const uint8_t *)addr(env, keys32), (const int32_t *)addr(env, nodes), n, nPassing);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(accmapFinish)(JNIEnv *env, jclass c, jlong accmap, jlongArray info) {
    int64_t v[4] = {0, 0, 0, 0};
    if (no_handle(env, JA(accmap)) || longs_short(env, info, 4, "info (4 x long)")) return;
    int rc = gs_accmap_finish(JA(accmap)->am, v);
    if (rc) return throw_gs(env, rc);
    JA(accmap)->n_entries = v[0];
    put_longs(env, info, v, 4, "info (4 x long)");
}

/* any of the three buffers may be null */
JNIEXPORT void JNICALL JNAME(accmapFetch)(JNIEnv *env, jclass c, jlong accmap, jobject keys32, jlong keys32Cap, jobject nodes, jlong nodesCap, jobject regions,
                                          jlong regionsCap) {
    if (no_handle(env, JA(accmap))) return;
    const int64_t n = JA(accmap)->n_entries;
    if (n < 0) return throw_gs(env, gs_accmap_fetch(JA(accmap)->am, NULL, NULL, NULL)); /* (in front of finish: the library's GS_E_STATE) */
    if ((keys32 && too_short(env, keys32, keys32Cap, 32 * n, "keys32 (entries x 32 bytes)")) || (nodes && too_short(env, nodes, nodesCap, n, "nodes (entries x int32)")) ||
        (regions && too_short(env, regions, regionsCap, JA(accmap)->n_nodes, "regions (nNodes x int32)")))
        return;
    int rc = gs_accmap_fetch(JA(accmap)->am, (uint8_t *)addr(env, keys32), (int32_t *)addr(env, nodes), (int32_t *)addr(env, regions));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(accmapLookup)(JNIEnv *env, jclass c, jlong accmap, jobject headers, jlong headersCap, jobject headerOff, jlong headerOffCap, jlong n,
                                           jboolean completeOnly, jobject nodeOut, jlong nodeOutCap) {
    if (no_handle(env, JA(accmap))) return;
    if (n < 0 || n == INT64_MAX) return throw_short(env, "n");
    const uint64_t *off = (const uint64_t *)addr(env, headerOff);
    if (too_short(env, headerOff, headerOffCap, n + 1, "headerOff (n + 1 x int64)") || too_short(env, nodeOut, nodeOutCap, n, "nodeOut (n x int32)")) return;
    if (off[n] > (uint64_t)INT64_MAX) return throw_short(env, "headerOff[n]");
    if (too_short(env, headers, headersCap, (int64_t)off[n], "headers (headerOff[n] bytes)")) return;
    int rc = gs_accmap_lookup(JA(accmap)->am, (const uint8_t *)addr(env, headers), off, n, GS_MEM_HOST, completeOnly ? 1 : 0, (int32_t *)addr(env, nodeOut));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(accmapLookupGenomes)(JNIEnv *env, jclass c, jlong accmap, jlong genomes, jboolean completeOnly, jobject nodeOut, jlong nodeOutCap) {
    if (no_handle(env, JA(accmap)) || no_handle(env, JG(genomes)) || too_short(env, nodeOut, nodeOutCap, JG(genomes)->n_records, "nodeOut (n_records x int32)")) return;
    int rc = gs_accmap_lookup_genomes(JA(accmap)->am, JG(genomes)->g, completeOnly ? 1 : 0, (int32_t *)addr(env, nodeOut));
    if (rc) throw_gs(env, rc);
}

JNIEXPORT jint JNICALL JNAME(accmapGetDevice)(JNIEnv *env, jclass c, jlong accmap) {
    int device = 0;
    if (no_handle(env, JA(accmap))) return 0;
    int rc = gs_accmap_get_device(JA(accmap)->am, &device);
    if (rc) throw_gs(env, rc);
    return device;
}

JNIEXPORT jint JNICALL JNAME(accmapGetNNodes)(JNIEnv *env, jclass c, jlong accmap) {
    int32_t n = 0;
    if (no_handle(env, JA(accmap))) return 0;
    int rc = gs_accmap_get_n_nodes(JA(accmap)->am, &n);
    if (rc) throw_gs(env, rc);
    return n;
}

JNIEXPORT void JNICALL JNAME(accmapDestroy)(JNIEnv *env, jclass c, jlong accmap) {
    if (!JA(accmap)) return;
    gs_accmap_destroy(JA(accmap)->am);
    free(JA(accmap));
}

/* gs_host_accmap_files; totals[5]: lines, passing, put, device_chunks, host_chunks; returns the map (0 with countOnly) */
JNIEXPORT jlong JNICALL JNAME(hostAccmapFiles)(JNIEnv *env, jclass c, jobjectArray paths, jint device, jboolean dna, jboolean rna, jboolean mrna,
                                               jobjectArray categories, jobjectArray statuses, jobject knownTaxids, jlong knownTaxidsCap, jint nNodes,
                                               jlong reserveEntries, jboolean countOnly, jlongArray totals) {
    StrArray p = {0, NULL, NULL}, cats = {0, NULL, NULL}, stats = {0, NULL, NULL};
    gs_accmap_cfg cfg;
    gs_host_accmap_totals t;
    gs_accmap *am = NULL;
    JAccmap *j = NULL;
    memset(&t, 0, sizeof(t));
    int rc = get_strings(env, paths, &p);
    if (!rc) rc = get_strings(env, categories, &cats);
    if (!rc) rc = get_strings(env, statuses, &stats);
    int thrown = !rc && (longs_short(env, totals, 5, "totals (5 x long)") ||
                         accmap_cfg(env, &cfg, dna, rna, mrna, &cats, &stats, knownTaxids, knownTaxidsCap, nNodes, reserveEntries));
    if (!rc && !thrown && !countOnly && !(j = (JAccmap *)calloc(1, sizeof(JAccmap)))) rc = GS_E_NOMEM;
    if (!rc && !thrown) rc = gs_host_accmap_files(p.c, (int)p.n, device, &cfg, countOnly ? 1 : 0, countOnly ? NULL : &am, &t);
    free_strings(env, &p);
    free_strings(env, &cats);
    free_strings(env, &stats);
    if (!thrown && (!rc || rc == GS_E_CANCELLED)) {
        const int64_t v[5] = {t.lines, t.passing, t.put, t.device_chunks, t.host_chunks};
        put_longs(env, totals, v, 5, "totals (5 x long)");
    }
    if (rc || thrown || !am) {
        free(j);
        if (rc && !thrown) throw_host(env, rc);
        return 0;
    }
    j->am = am;
    j->n_entries = t.put;
    j->n_nodes = nNodes;
    return (jlong)(intptr_t)j;
}

/* ---- gs_asmsum ---- */
static int asmsum_cfg(JNIEnv *env, gs_asmsum_cfg *cfg, jobject known, jlong knownCap, jint nNodes, jobject filter, jlong filterCap, jint qualityMask,
                      jboolean referenceOnly, jboolean useSpeciesTaxid, jlong reserve) {
    if (too_short(env, known, knownCap, nNodes, "knownTaxids (nNodes x int32)") || (filter && too_short(env, filter, filterCap, nNodes, "filter (nNodes bytes)")))
        return 1;
    memset(cfg, 0, sizeof(*cfg));
    cfg->n_nodes = nNodes;
    cfg->known_taxids = (const int32_t *)addr(env, known);
    cfg->filter = (const uint8_t *)addr(env, filter);
    cfg->quality_mask = qualityMask;
    cfg->reference_only = referenceOnly ? 1 : 0;
    cfg->use_species_taxid = useSpeciesTaxid ? 1 : 0;
    cfg->reserve_entries = reserve;
    return 0;
}

JNIEXPORT jlong JNICALL JNAME(asmsumCreate)(JNIEnv *env, jclass c, jint device, jobject knownTaxids, jlong knownTaxidsCap, jint nNodes, jobject filter,
                                            jlong filterCap, jint qualityMask, jboolean referenceOnly, jboolean useSpeciesTaxid, jlong reserveEntries) {
    gs_asmsum_cfg cfg;
    if (asmsum_cfg(env, &cfg, knownTaxids, knownTaxidsCap, nNodes, filter, filterCap, qualityMask, referenceOnly, useSpeciesTaxid, reserveEntries)) return 0;
    JAsmsum *j = (JAsmsum *)calloc(1, sizeof(JAsmsum));
    int rc = j ? gs_asmsum_create(&j->as, device, &cfg) : GS_E_NOMEM;
    if (rc) {
        free(j);
        return throw_gs(env, rc), 0;
    }
    j->n_picked = -1;
    return (jlong)(intptr_t)j;
}

JNIEXPORT void JNICALL JNAME(asmsumSubmit)(JNIEnv *env, jclass c, jlong asmsum, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray report) {
    int64_t r[8] = {0};
    if (no_handle(env, JS(asmsum)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, report, 8, "report (8 x long)")) return;
    int rc = gs_asmsum_submit(JS(asmsum)->as, (const uint8_t *)addr(env, text), nBytes, GS_MEM_HOST, last ? 1 : 0, r);
    if (rc) return throw_gs(env, rc);
    put_longs(env, report, r, 8, "report (8 x long)");
}

JNIEXPORT void JNICALL JNAME(asmsumAppend)(JNIEnv *env, jclass c, jlong asmsum, jobject nodes, jlong nodesCap, jobject quality, jlong qualityCap, jobject isRef,
                                           jlong isRefCap, jobject lines, jlong linesCap, jobject strOff, jlong strOffCap, jobject pool, jlong poolCap, jlong n,
                                           jlong nCounted, jlong nLines) {
    if (no_handle(env, JS(asmsum))) return;
    if (n < 0 || n > (INT64_MAX >> 4)) return throw_short(env, "n");
    const uint64_t *off = (const uint64_t *)addr(env, strOff);
    if (too_short(env, nodes, nodesCap, n, "nodes (n x int32)") || too_short(env, quality, qualityCap, n, "quality (n bytes)") ||
        too_short(env, isRef, isRefCap, n, "isRef (n bytes)") || too_short(env, lines, linesCap, n, "lines (n x int64)") ||
        too_short(env, strOff, strOffCap, 3 * n + 1, "strOff (3 n + 1 x int64)"))
        return;
    if (off && (off[3 * n] > (uint64_t)INT64_MAX || too_short(env, pool, poolCap, (int64_t)off[3 * n], "pool (strOff[3 n] bytes)"))) return;
    int rc = gs_asmsum_append(JS(asmsum)->as, (const int32_t *)addr(env, nodes), (const uint8_t *)addr(env, quality), (const uint8_t *)addr(env, isRef),
                              (const int64_t *)addr(env, lines), off, (const uint8_t *)addr(env, pool), n, nCounted, nLines);
    if (rc) throw_gs(env, rc);
}

JNIEXPORT void JNICALL JNAME(asmsumFinish)(JNIEnv *env, jclass c, jlong asmsum, jint maxPerNode, jlongArray info) {
    int64_t v[4] = {0, 0, 0, 0};
    if (no_handle(env, JS(asmsum)) || longs_short(env, info, 4, "info (4 x long)")) return;
    int rc = gs_asmsum_finish(JS(asmsum)->as, maxPerNode, v);
    if (rc) return throw_gs(env, rc);
    JS(asmsum)->n_picked = v[1];
    put_longs(env, info, v, 4, "info (4 x long)");
}

/* any buffer may be null; pool needs strOff[3 x picked] bytes: fetch strOff first, as with the C call */
JNIEXPORT void JNICALL JNAME(asmsumFetch)(JNIEnv *env, jclass c, jlong asmsum, jobject nodes, jlong nodesCap, jobject quality, jlong qualityCap, jobject isRef,
                                          jlong isRefCap, jobject lines, jlong linesCap, jobject strOff, jlong strOffCap, jobject pool, jlong poolCap) {
    if (no_handle(env, JS(asmsum))) return;
    const int64_t m = JS(asmsum)->n_picked;
    if (m < 0) return throw_gs(env, gs_asmsum_fetch(JS(asmsum)->as, NULL, NULL, NULL, NULL, NULL, NULL)); /* (the library's GS_E_STATE) */
    if ((nodes && too_short(env, nodes, nodesCap, m, "nodes (picked x int32)")) || (quality && too_short(env, quality, qualityCap, m, "quality (picked bytes)")) ||
        (isRef && too_short(env, isRef, isRefCap, m, "isRef (picked bytes)")) || (lines && too_short(env, lines, linesCap, m, "lines (picked x int64)")) ||
        (strOff && too_short(env, strOff, strOffCap, 3 * m + 1, "strOff (3 x picked + 1 x int64)")))
        return;
    int rc = GS_OK;
    if (pool) {
        uint64_t *off = (uint64_t *)calloc((size_t)(3 * m + 1), sizeof(uint64_t));
        rc = off ? gs_asmsum_fetch(JS(asmsum)->as, NULL, NULL, NULL, NULL, off, NULL) : GS_E_NOMEM;
        const int64_t bytes = rc ? 0 : (int64_t)off[3 * m];
        free(off);
        if (rc) return throw_gs(env, rc);
        if (too_short(env, pool, poolCap, bytes, "pool (strOff[3 x picked] bytes)")) return;
    }
    rc = gs_asmsum_fetch(JS(asmsum)->as, (int32_t *)addr(env, nodes), (uint8_t *)addr(env, quality), (uint8_t *)addr(env, isRef), (int64_t *)addr(env, lines),
                         (uint64_t *)addr(env, strOff), (uint8_t *)addr(env, pool));
    if (rc) throw_gs(env, rc);
}

/* returns the name's length; min(length, outCap) bytes are written */
JNIEXPORT jlong JNICALL JNAME(asmsumFileName)(JNIEnv *env, jclass c, jobject ftp, jlong ftpCap, jlong n, jobject out, jlong outCap) {
    if (too_short(env, ftp, ftpCap, n, "ftp (n bytes)")) return 0;
    if (outCap < 0 || (outCap > 0 && !addr(env, out))) return throw_short(env, "out (outCap bytes)"), 0;
    int64_t len = gs_asmsum_file_name((const uint8_t *)addr(env, ftp), n, (uint8_t *)addr(env, out), outCap);
    if (len < 0) return throw_gs(env, (int)len), 0;
    return (jlong)len;
}

JNIEXPORT jint JNICALL JNAME(asmsumGetDevice)(JNIEnv *env, jclass c, jlong asmsum) {
    int device = 0;
    if (no_handle(env, JS(asmsum))) return 0;
    int rc = gs_asmsum_get_device(JS(asmsum)->as, &device);
    if (rc) throw_gs(env, rc);
    return device;
}

JNIEXPORT void JNICALL JNAME(asmsumDestroy)(JNIEnv *env, jclass c, jlong asmsum) {
    if (!JS(asmsum)) return;
    gs_asmsum_destroy(JS(asmsum)->as);
    free(JS(asmsum));
}

/* gs_host_asmsum_files; totals[7]: lines, counted, kept, picked, nodes, device_chunks, host_chunks; returns the finished handle */
JNIEXPORT jlong JNICALL JNAME(hostAsmsumFiles)(JNIEnv *env, jclass c, jobjectArray paths, jint device, jobject knownTaxids, jlong knownTaxidsCap, jint nNodes,
                                               jobject filter, jlong filterCap, jint qualityMask, jboolean referenceOnly, jboolean useSpeciesTaxid,
                                               jlong reserveEntries, jint maxPerNode, jlongArray totals) {
    StrArray p = {0, NULL, NULL};
    gs_asmsum_cfg cfg;
    gs_host_asmsum_totals t;
    gs_asmsum *as = NULL;
    memset(&t, 0, sizeof(t));
    if (longs_short(env, totals, 7, "totals (7 x long)") ||
        asmsum_cfg(env, &cfg, knownTaxids, knownTaxidsCap, nNodes, filter, filterCap, qualityMask, referenceOnly, useSpeciesTaxid, reserveEntries))
        return 0;
    JAsmsum *j = (JAsmsum *)calloc(1, sizeof(JAsmsum));
    int rc = j ? get_strings(env, paths, &p) : GS_E_NOMEM;
    if (!rc) rc = gs_host_asmsum_files(p.c, (int)p.n, device, &cfg, maxPerNode, &as, &t);
    free_strings(env, &p);
    if (!rc || rc == GS_E_CANCELLED) {
        const int64_t v[7] = {t.lines, t.counted, t.kept, t.picked, t.nodes, t.device_chunks, t.host_chunks};
        put_longs(env, totals, v, 7, "totals (7 x long)");
    }
    if (rc || !as) {
        free(j);
        if (rc) throw_host(env, rc);
        return 0;
    }
    j->as = as;
    j->n_picked = t.picked;
    return (jlong)(intptr_t)j;
}

/* ---- gs_taxtree ---- */
JNIEXPORT jlong JNICALL JNAME(taxtreeCreate)(JNIEnv *env, jclass c, jint device) {
    JTaxtree *j = (JTaxtree *)calloc(1, sizeof(JTaxtree));
    int rc = j ? gs_taxtree_create(&j->t, device) : GS_E_NOMEM;
    if (rc) {
        free(j);
        return throw_gs(env, rc), 0;
    }
    j->n_nodes = j->n_reached = -1;
    return (jlong)(intptr_t)j;
}

JNIEXPORT void JNICALL JNAME(taxtreeSubmitNodes)(JNIEnv *env, jclass c, jlong taxtree, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray report) {
    int64_t r[8] = {0};
    if (no_handle(env, JT(taxtree)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, report, 8, "report (8 x long)")) return;
    int rc = gs_taxtree_submit_nodes(JT(taxtree)->t, (const uint8_t *)addr(env, text), nBytes, GS_MEM_HOST, last ? 1 : 0, r);
    if (rc) return throw_gs(env, rc);
    put_longs(env, report, r, 8, "report (8 x long)");
}

JNIEXPORT void JNICALL JNAME(taxtreeAppendNodes)(JNIEnv *env, jclass c, jlong taxtree, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray report) {
    int64_t r[8] = {0};
    if (no_handle(env, JT(taxtree)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, report, 8, "report (8 x long)")) return;
    int rc = gs_taxtree_append_nodes(JT(taxtree)->t, (const uint8_t *)addr(env, text), nBytes, last ? 1 : 0, r);
    if (rc) return throw_gs(env, rc);
    put_longs(env, report, r, 8, "report (8 x long)");
}

JNIEXPORT void JNICALL JNAME(taxtreeFinishNodes)(JNIEnv *env, jclass c, jlong taxtree, jlongArray info) {
    int64_t v[8] = {0};
    if (no_handle(env, JT(taxtree)) || longs_short(env, info, 8, "info (8 x long)")) return;
    int rc = gs_taxtree_finish_nodes(JT(taxtree)->t, v);
    if (rc) return throw_gs(env, rc);
    JT(taxtree)->n_nodes = v[0];
    JT(taxtree)->n_reached = v[1];
    put_longs(env, info, v, 8, "info (8 x long)");
}

JNIEXPORT void JNICALL JNAME(taxtreeSubmitNames)(JNIEnv *env, jclass c, jlong taxtree, jobject text, jlong textCap, jlong nBytes, jboolean last, jlongArray report) {
    int64_t r[8] = {0};
    if (no_handle(env, JT(taxtree)) || too_short(env, text, textCap, nBytes, "text (nBytes)") || longs_short(env, report, 8, "report (8 x long)")) return;
    int rc = gs_taxtree_submit_names(JT(taxtree)->t, (const uint8_t *)addr(env, text), nBytes, GS_MEM_HOST, last ? 1 : 0, r);
    if (rc) return throw_gs(env, rc);
    put_longs(env, report, r, 8, "report (8 x long)");
}

JNIEXPORT void JNICALL JNAME(taxtreeAppendNames)(JNIEnv *env, jclass c, jlong taxtree, jobject text, jlong textCap, jlong nBytes, jboolean last) {
    if (no_handle(env, JT(taxtree)) || too_short(env, text, textCap, nBytes, "text (nBytes)")) return;
    int rc = gs_taxtree_append_names(JT(taxtree)->t, (const uint8_t *)addr(env, text), nBytes, last ? 1 : 0);
    if (rc) throw_gs(env, rc);
}

/* 1 (and the exception is pending): the tree is not finished -- raised through the library's own GS_E_STATE */
static int tree_unfinished(JNIEnv *env, jlong taxtree) {
    if (no_handle(env, JT(taxtree))) return 1;
    if (JT(taxtree)->n_nodes >= 0) return 0;
    int rc = gs_taxtree_fetch(JT(taxtree)->t, NULL, NULL, NULL, NULL, NULL, NULL);
    if (rc)
        throw_gs(env, rc);
    else
        throw_short(env, "the tree has not been finished through this handle");
    return 1;
}

/* any of the six buffers may be null */
JNIEXPORT void JNICALL JNAME(taxtreeFetch)(JNIEnv *env, jclass c, jlong taxtree, jobject taxids, jlong taxidsCap, jobject parent, jlong parentCap, jobject depth,
                                           jlong depthCap, jobject position, jlong positionCap, jobject subtree, jlong subtreeCap, jobject rank, jlong rankCap) {
    if (tree_unfinished(env, taxtree)) return;
    const int64_t n = JT(taxtree)->n_nodes;
    if ((taxids && too_short(env, taxids, taxidsCap, n, "taxids (nodes x int32)")) || (parent && too_short(env, parent, parentCap, n, "parent (nodes x int32)")) ||
        (depth && too_short(env, depth, depthCap, n, "depth (nodes x int32)")) || (position && too_short(env, position, positionCap, n, "position (nodes x int32)")) ||
        (subtree && too_short(env, subtree, subtreeCap, n, "subtree (nodes x int32)")) || (rank && too_short(env, rank, rankCap, n, "rank (nodes x int32)")))
        return;
    int rc = gs_taxtree_fetch(JT(taxtree)->t, (int32_t *)addr(env, taxids), (int32_t *)addr(env, parent), (int32_t *)addr(env, depth), (int32_t *)addr(env, position),
                              (int32_t *)addr(env, subtree), (int32_t *)addr(env, rank));
    if (rc) throw_gs(env, rc);
}

/* offsets: nodes + 1 x int64; bytes: null for the offsets alone, else bytesCap is the library's cap */
JNIEXPORT void JNICALL JNAME(taxtreeFetchNames)(JNIEnv *env, jclass c, jlong taxtree, jobject offsets, jlong offsetsCap, jobject bytes, jlong bytesCap) {
    if (tree_unfinished(env, taxtree) || too_short(env, offsets, offsetsCap, JT(taxtree)->n_nodes + 1, "offsets (nodes + 1 x int64)")) return;
    if (bytes && bytesCap < 0) return throw_short(env, "bytes");
    int rc = gs_taxtree_fetch_names(JT(taxtree)->t, (int64_t *)addr(env, offsets), (uint8_t *)addr(env, bytes), bytes ? bytesCap : 0);
    if (rc) throw_gs(env, rc);
}

/* returns the count; requested / excluded: node indices, null with n = 0 */
JNIEXPORT jlong JNICALL JNAME(taxtreeSelect)(JNIEnv *env, jclass c, jlong taxtree, jintArray requested, jlong nRequested, jintArray excluded, jlong nExcluded,
                                             jint cutRank, jobject out, jlong outCap) {
    int64_t count = 0;
    if (tree_unfinished(env, taxtree) || too_short(env, out, outCap, JT(taxtree)->n_nodes, "out (nodes bytes)")) return 0;
    if (nRequested < 0 || nExcluded < 0 || (nRequested > 0 && (!requested || (*env)->GetArrayLength(env, requested) < nRequested)) ||
        (nExcluded > 0 && (!excluded || (*env)->GetArrayLength(env, excluded) < nExcluded)))
        return throw_short(env, "requested / excluded"), 0;
    jint *rq = requested ? (*env)->GetIntArrayElements(env, requested, NULL) : NULL;
    jint *ex = excluded ? (*env)->GetIntArrayElements(env, excluded, NULL) : NULL;
    int rc = gs_taxtree_select(JT(taxtree)->t, (const int32_t *)rq, nRequested, (const int32_t *)ex, nExcluded, cutRank, (uint8_t *)addr(env, out), &count);
    if (rq) (*env)->ReleaseIntArrayElements(env, requested, rq, JNI_ABORT);
    if (ex) (*env)->ReleaseIntArrayElements(env, excluded, ex, JNI_ABORT);
    if (rc) return throw_gs(env, rc), 0;
    return (jlong)count;
}

/* flagged: nodes x flagBytes (1 or 4) in host memory; the four outputs (any may be null): room for the nodes the root reaches; returns n_small */
JNIEXPORT jint JNICALL JNAME(taxtreeSmall)(JNIEnv *env, jclass c, jlong taxtree, jobject flagged, jlong flaggedCap, jint flagBytes, jobject nodeOfVi,
                                           jlong nodeOfViCap, jobject parentVi, jlong parentViCap, jobject depth, jlong depthCap, jobject position, jlong positionCap) {
    int32_t n_small = 0;
    if (tree_unfinished(env, taxtree)) return 0;
    const int64_t n = JT(taxtree)->n_nodes, m = JT(taxtree)->n_reached;
    if (flagBytes != 1 && flagBytes != 4) return throw_short(env, "flagBytes (1 or 4)"), 0;
    if (too_short(env, flagged, flaggedCap, n, "flagged (nodes elements)") || (nodeOfVi && too_short(env, nodeOfVi, nodeOfViCap, m, "nodeOfVi (reached x int32)")) ||
        (parentVi && too_short(env, parentVi, parentViCap, m, "parentVi (reached x int32)")) || (depth && too_short(env, depth, depthCap, m, "depth (reached x int32)")) ||
        (position && too_short(env, position, positionCap, m, "position (reached x int32)")))
        return 0;
    int rc = gs_taxtree_small(JT(taxtree)->t, addr(env, flagged), flagBytes, GS_MEM_HOST, &n_small, (int32_t *)addr(env, nodeOfVi), (int32_t *)addr(env, parentVi),
                              (int32_t *)addr(env, depth), (int32_t *)addr(env, position));
    if (rc) return throw_gs(env, rc), 0;
    return n_small;
}

/* regions: nodes x int32 in host memory; inclusive (nodes x int32) and below (nSelected x int32) may be null; returns n_below */
JNIEXPORT jlong JNICALL JNAME(taxtreeRegionsBelow)(JNIEnv *env, jclass c, jlong taxtree, jobject regions, jlong regionsCap, jintArray selected, jlong nSelected,
                                                   jint limit, jint checkRank, jobject inclusive, jlong inclusiveCap, jobject below, jlong belowCap) {
    int64_t n_below = 0;
    if (tree_unfinished(env, taxtree)) return 0;
    const int64_t n = JT(taxtree)->n_nodes;
    if (too_short(env, regions, regionsCap, n, "regions (nodes x int32)") || (inclusive && too_short(env, inclusive, inclusiveCap, n, "inclusive (nodes x int32)")) ||
        (below && too_short(env, below, belowCap, nSelected, "below (nSelected x int32)")))
        return 0;
    if (nSelected < 0 || (nSelected > 0 && (!selected || (*env)->GetArrayLength(env, selected) < nSelected))) return throw_short(env, "selected"), 0;
    jint *sel = selected ? (*env)->GetIntArrayElements(env, selected, NULL) : NULL;
    int rc = gs_taxtree_regions_below(JT(taxtree)->t, (const int32_t *)addr(env, regions), GS_MEM_HOST, (const int32_t *)sel, nSelected, limit, checkRank,
                                      (int32_t *)addr(env, inclusive), (int32_t *)addr(env, below), &n_below);
    if (sel) (*env)->ReleaseIntArrayElements(env, selected, sel, JNI_ABORT);
    if (rc) return throw_gs(env, rc), 0;
    return (jlong)n_below;
}

/* counts[2]: n_requested, n_excluded -- how many there are; at most cap of each are written */
JNIEXPORT void JNICALL JNAME(taxtreeReadTaxids)(JNIEnv *env, jclass c, jobject text, jlong textCap, jlong nBytes, jobject requested, jlong requestedCap,
                                                jobject excluded, jlong excludedCap, jlong cap, jlongArray counts) {
    int64_t v[2] = {0, 0};
    if (too_short(env, text, textCap, nBytes, "text (nBytes)") || too_short(env, requested, requestedCap, cap, "requested (cap x int32)") ||
        too_short(env, excluded, excludedCap, cap, "excluded (cap x int32)") || longs_short(env, counts, 2, "counts (2 x long)"))
        return;
    int rc = gs_taxtree_read_taxids((const uint8_t *)addr(env, text), nBytes, (int32_t *)addr(env, requested), &v[0], (int32_t *)addr(env, excluded), &v[1], cap);
    if (rc) return throw_gs(env, rc);
    put_longs(env, counts, v, 2, "counts (2 x long)");
}

JNIEXPORT jint JNICALL JNAME(taxtreeGetDevice)(JNIEnv *env, jclass c, jlong taxtree) {
    int device = 0;
    if (no_handle(env, JT(taxtree))) return 0;
    int rc = gs_taxtree_get_device(JT(taxtree)->t, &device);
    if (rc) throw_gs(env, rc);
    return device;
}

JNIEXPORT void JNICALL JNAME(taxtreeDestroy)(JNIEnv *env, jclass c, jlong taxtree) {
    if (!JT(taxtree)) return;
    gs_taxtree_destroy(JT(taxtree)->t);
    free(JT(taxtree));
}

/* gs_host_taxtree_files; namesPath may be null; report[8] as the C call's; returns the finished tree */
JNIEXPORT jlong JNICALL JNAME(hostTaxtreeFiles)(JNIEnv *env, jclass c, jint device, jstring nodesPath, jstring namesPath, jlongArray report) {
    int64_t r[8] = {0};
    gs_taxtree *t = NULL;
    if (longs_short(env, report, 8, "report (8 x long)")) return 0;
    JTaxtree *j = (JTaxtree *)calloc(1, sizeof(JTaxtree));
    const char *nodes = nodesPath ? (*env)->GetStringUTFChars(env, nodesPath, NULL) : NULL;
    const char *names = namesPath ? (*env)->GetStringUTFChars(env, namesPath, NULL) : NULL;
    int rc = j ? gs_host_taxtree_files(device, nodes, names, &t, r) : GS_E_NOMEM;
    if (nodes) (*env)->ReleaseStringUTFChars(env, nodesPath, nodes);
    if (names) (*env)->ReleaseStringUTFChars(env, namesPath, names);
    if (!rc || rc == GS_E_CANCELLED) put_longs(env, report, r, 8, "report (8 x long)");
    if (rc || !t) {
        free(j);
        if (rc) throw_host(env, rc);
        return 0;
    }
    j->t = t;
    j->n_nodes = r[4];
    j->n_reached = r[5];
    return (jlong)(intptr_t)j;
}

/* gs_host_read_taxids_file; counts[2] as taxtreeReadTaxids */
JNIEXPORT void JNICALL JNAME(hostReadTaxidsFile)(JNIEnv *env, jclass c, jstring path, jobject requested, jlong requestedCap, jobject excluded, jlong excludedCap,
                                                 jlong cap, jlongArray counts) {
    int64_t v[2] = {0, 0};
    if (too_short(env, requested, requestedCap, cap, "requested (cap x int32)") || too_short(env, excluded, excludedCap, cap, "excluded (cap x int32)") ||
        longs_short(env, counts, 2, "counts (2 x long)"))
        return;
    const char *p = path ? (*env)->GetStringUTFChars(env, path, NULL) : NULL;
    int rc = gs_host_read_taxids_file(p, (int32_t *)addr(env, requested), &v[0], (int32_t *)addr(env, excluded), &v[1], cap);
    if (p) (*env)->ReleaseStringUTFChars(env, path, p);
    if (rc) return throw_host(env, rc);
    put_longs(env, counts, v, 2, "counts (2 x long)");
}

/* gs_host_genome_files_into: accmap is an accmap* native's handle or 0; nodeOfFile null or one entry per path; kind / handle: GS_HOST_INTO_* and the
 * handle of dbSizeBegin / dbBuildBegin / dbUpdateBegin* / dbQualityBegin; totals[7]: records, kept_records, text_bytes, kept_bases, chunks, host_chunks,
 * max_line_bytes */
JNIEXPORT void JNICALL JNAME(hostGenomeFilesInto)(JNIEnv *env, jclass c, jobjectArray paths, jint device, jlong accmap, jboolean completeOnly, jintArray nodeOfFile,
                                                  jobject viOfNode, jlong viOfNodeCap, jint nNodes, jint kind, jlong handle, jboolean update, jlongArray totals) {
    StrArray p = {0, NULL, NULL};
    gs_host_genome_totals t;
    memset(&t, 0, sizeof(t));
    if (too_short(env, viOfNode, viOfNodeCap, nNodes, "viOfNode (nNodes x int32)") || longs_short(env, totals, 7, "totals (7 x long)")) return;
    if (nodeOfFile && (*env)->GetArrayLength(env, nodeOfFile) < (paths ? (*env)->GetArrayLength(env, paths) : 0))
        return throw_short(env, "nodeOfFile (one per path)");
    int rc = get_strings(env, paths, &p);
    jint *nof = nodeOfFile ? (*env)->GetIntArrayElements(env, nodeOfFile, NULL) : NULL;
    if (!rc)
        rc = gs_host_genome_files_into(p.c, (int)p.n, device, JA(accmap) ? JA(accmap)->am : NULL, completeOnly ? 1 : 0, (const int32_t *)nof,
                                       (const int32_t *)addr(env, viOfNode), nNodes, kind, (void *)(intptr_t)handle, update ? 1 : 0, &t);
    if (nof) (*env)->ReleaseIntArrayElements(env, nodeOfFile, nof, JNI_ABORT);
    free_strings(env, &p);
    if (!rc || rc == GS_E_CANCELLED) {
        const int64_t v[7] = {t.records, t.kept_records, t.text_bytes, t.kept_bases, t.chunks, t.host_chunks, t.max_line_bytes};
        put_longs(env, totals, v, 7, "totals (7 x long)");
    }
    if (rc) throw_host(env, rc);
}
