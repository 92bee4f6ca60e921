// gs_api.cpp -- C ABI (include/gsgpu.h) over the gfx950 kernels: host-side table build, HBM residency,
// stream/event plumbing.  No CPU fallback exists: every entry point needs a HIP device and fails with
// GS_E_NODEVICE / GS_E_HIP otherwise.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "gs_absmod.h"
#include "gs_asmsumparse.h"
#include "gs_checksum.h"
#include "gs_indexfile.h"
#include "gs_launch.h"
#include "gs_layout.h"
#include "gs_params.h"
#include "gs_prefilter.h"
#include "gs_taxparse.h"

// ---------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// the fence of an entry point whose host allocations (std::vector, std::string) can throw: `int f(...) try { ... } GS_API_CATCH`
// (nothing may leave through the C ABI)
#define GS_API_CATCH                                                                  \
    catch (const std::bad_alloc &) { return fail(GS_E_NOMEM, "out of host memory"); } \
    catch (const std::exception &e) { return fail(GS_E_INVALID, std::string("unexpected exception: ") + e.what()); }

static int hip_fail(hipError_t e, const std::string &where) {
    return fail(e == hipErrorOutOfMemory ? GS_E_NOMEM : GS_E_HIP, where + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e_ = (expr);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

// a chain of device steps joined by &&: the first failure is the call's error, `who (what): reason`
struct HipSteps {
    const char *who;
    int rc = GS_OK;
    bool operator()(hipError_t e, const char *what) {
        if (e != hipSuccess && rc == GS_OK) rc = hip_fail(e, std::string(who) + " (" + what + ")");
        return e == hipSuccess;
    }
};

static double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

extern "C" const char *gs_last_error(void) { return g_err.c_str(); }

extern "C" const char *gs_strerror(int code) {
    switch (code) {
    case GS_OK: return "ok";
    case GS_E_INVALID: return "invalid argument";
    case GS_E_NOMEM: return "out of memory";
    case GS_E_HIP: return "HIP runtime error";
    case GS_E_UNSUPPORTED: return "unsupported";
    case GS_E_STATE: return "invalid call order";
    case GS_E_NODEVICE: return "no usable gfx950 device";
    case GS_E_IO: return "file input/output failed";
    case GS_E_CANCELLED: return "cancelled";
    default: return "unknown error";
    }
}

extern "C" int gs_abi_version(void) { return GS_ABI_VERSION; }

extern "C" int gs_device_count(int *n) {
    if (!n) return fail(GS_E_INVALID, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *n = 0;
        return fail(GS_E_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *n = c;
    return GS_OK;
}

static int use_device(int device) {
    int c = 0;
    int rc = gs_device_count(&c);
    if (rc) return rc;
    if (device < 0 || device >= c) return fail(GS_E_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// store build
// ---------------------------------------------------------------------------------------------------
struct gs_db {
    int device = 0;
    gs_db_info info{};
    GsDbDev dev{};
    u64 *d_table = nullptr;
    u64 *d_gate = nullptr;
    uint32_t *d_mgate = nullptr;
    u64 *d_rec = nullptr;       // super-k-mer records (gs_layout.h), GS_REC_WORDS words per bucket
    int64_t n_rec = 0;          // record buckets (a power of two) or 0
    int32_t *d_tree = nullptr;  // parent | depth | tin | tout
    int64_t n_slots() const { return info.n_buckets * GS_SLOTS_PER_BUCKET; }
    int n_cu = 256;
    struct gs_run *unique_owner = nullptr;  // the slots' seen bits belong to one unique-counting run at a time
    // Runs keep a pointer to their store.  A host with garbage-collected wrappers (Java finalizers, Python __del__) may
    // destroy the store before its runs: gs_db_destroy then only marks it, and the last gs_match_destroy frees it.
    int live_runs = 0;
    bool destroy_pending = false;
    // striped store (gs_layout.h, GsDbDev::rec_biased): d_rec is THIS handle's stripe, buckets [rec_first, rec_first +
    // rec_local) of the n_rec buckets; stripe_base[q] = where this process sees stripe q
    int n_parts = 0, part = 0;
    int64_t rec_first = 0, rec_local = 0;
    int64_t tab_first = 0, tab_local = 0;      // its buckets of the overflow table: they follow the record lines in d_rec
    const u64 *stripe_base[GS_MAX_STRIPES] = {};
    unsigned present = 0;                      // bit q: stripe q is known
    std::shared_ptr<struct StripeGroup> group; // all stripes in one process: they are freed with the last handle
    std::vector<void *> ipc_opened;            // stripes of other processes (hipIpcOpenMemHandle)
    // the 15-mer filter of the store (gs_prefilter.h): both levels in one allocation (exact level first), built by the first run
    // that may use it (db_ensure_prefilter) and never written to the store file
    uint32_t *d_pf = nullptr;
    int64_t pf_set = -1;  // |S|, the set bits of the exact level; -1: not built yet
    bool striped() const { return n_parts > 1; }
    bool complete() const { return n_parts <= 1 || present == (1u << n_parts) - 1u; }
};

struct StripeGroup {
    std::vector<std::pair<int, void *>> allocs;
    ~StripeGroup() {
        for (auto &a : allocs) {
            hipSetDevice(a.first);
            gs_dev_free(a.second);
        }
    }
};

static void db_set_stripe(gs_db *db, int q, const u64 *base) {
    db->stripe_base[q] = base;
    db->present |= 1u << q;
    // (biased: the kernels add bucket * GS_REC_WORDS with the GLOBAL bucket number)
    const size_t first = (size_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q);
    const size_t local = (size_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q + 1) - first;
    db->dev.rec_biased[q] = base - first * GS_REC_WORDS;
    db->dev.tab_biased[q] = base + local * GS_REC_WORDS -
                            (size_t)gs_tab_stripe_first(db->dev.bucket_bits, (uint32_t)db->n_parts, (uint32_t)q) * GS_SLOTS_PER_BUCKET;
}
// the table buckets of stripe q as this process sees them
static const u64 *stripe_table(const gs_db *db, int q, int64_t *first, int64_t *local) {
    const int64_t rf = (int64_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q);
    const int64_t rl = (int64_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q + 1) - rf;
    *first = (int64_t)gs_tab_stripe_first(db->dev.bucket_bits, (uint32_t)db->n_parts, (uint32_t)q);
    *local = (int64_t)gs_tab_stripe_first(db->dev.bucket_bits, (uint32_t)db->n_parts, (uint32_t)q + 1) - *first;
    return db->stripe_base[q] + (size_t)rl * GS_REC_WORDS;
}

static void db_free(gs_db *db) {
    hipSetDevice(db->device);
    for (void *p : db->ipc_opened) hipIpcCloseMemHandle(p);
    if (!db->striped()) gs_dev_free(db->d_table);  // (a stripe's table buckets live behind its record lines)
    gs_dev_free(db->d_gate);
    gs_dev_free(db->d_mgate);
    gs_dev_free(db->d_pf);
    if (!db->group) gs_dev_free(db->d_rec);
    gs_dev_free(db->d_tree);
    delete db;
}

// reference (interleaved, first base in the top bits) -> forward planes; also reports reachability:
// the reference only ever queries max(fwd, revcomp) (CGAT.java:145-147), so a stored key that is smaller
// than its reverse complement can never be hit.
static inline bool java_to_planes(u64 x, int k, uint32_t &hi, uint32_t &lo) {
    hi = lo = 0;
    u64 rc = 0;
    for (int i = 0; i < k; i++) {
        uint32_t c = (uint32_t)(x >> (2 * (k - 1 - i))) & 3u;
        hi |= (c >> 1) << i;
        lo |= (c & 1u) << i;
        rc |= (u64)(c ^ 1u) << (2 * i);  // base i complemented lands at position k-1-i from the top
    }
    return x >= rc;
}

static int bits_for(u64 v) {
    int b = 0;
    while (v) {
        b++;
        v >>= 1;
    }
    return b;
}

static int db_create_impl(gs_db **out, int device, int k, int64_t n, const int64_t *kmers, const int32_t *vidx,
                          int32_t n_values, const int32_t *parent_vi, int n_parts, int part, bool fused, int stripes = 1,
                          const int *stripe_devices = nullptr, int stripe_only = -1);
static int db_self_check(gs_db *db);

extern "C" int gs_db_create(gs_db **out, int device, int k, int64_t n, const int64_t *kmers, const int32_t *vidx,
                            int32_t n_values, const int32_t *parent_vi) try {
    return db_create_impl(out, device, k, n, kmers, vidx, n_values, parent_vi, 1, 0, true);
}
GS_API_CATCH

extern "C" int gs_db_create_part(gs_db **out, int device, int k, int64_t n, const int64_t *kmers, const int32_t *vidx,
                                 int32_t n_values, const int32_t *parent_vi, int n_parts, int part) try {
    if (n_parts < 1 || part < 0 || part >= n_parts) return fail(GS_E_INVALID, "bad partition");
    return db_create_impl(out, device, k, n, kmers, vidx, n_values, parent_vi, n_parts, part, false);
}
GS_API_CATCH

// ---- striped store (include/gsgpu.h)
extern "C" int gs_db_create_striped(gs_db **out, const int *devices, int n_stripes, int k, int64_t n, const int64_t *kmers,
                                    const int32_t *vidx, int32_t n_values, const int32_t *parent_vi) try {
    if (!out || !devices || n_stripes < 2 || n_stripes > GS_MAX_STRIPES) return fail(GS_E_INVALID, "a striped store spans 2..8 devices");
    for (int p = 0; p < n_stripes; p++) {
        out[p] = nullptr;
        const int rc = use_device(devices[p]);
        if (rc) return rc;
    }
    return db_create_impl(out, devices[0], k, n, kmers, vidx, n_values, parent_vi, 1, 0, true, n_stripes, devices, -1);
}
GS_API_CATCH

extern "C" int gs_db_create_stripe(gs_db **out, int device, int n_stripes, int stripe, int k, int64_t n, const int64_t *kmers,
                                   const int32_t *vidx, int32_t n_values, const int32_t *parent_vi) try {
    if (!out || n_stripes < 2 || n_stripes > GS_MAX_STRIPES || stripe < 0 || stripe >= n_stripes)
        return fail(GS_E_INVALID, "a striped store spans 2..8 devices");
    return db_create_impl(out, device, k, n, kmers, vidx, n_values, parent_vi, 1, 0, true, n_stripes, nullptr, stripe);
}
GS_API_CATCH

extern "C" int gs_db_stripe_export(gs_db *db, void *handle) {
    if (!db || !handle) return fail(GS_E_INVALID, "NULL argument");
    if (!db->striped() || db->group) return fail(GS_E_STATE, "not a stripe of gs_db_create_stripe");
    static_assert(sizeof(hipIpcMemHandle_t) <= GS_STRIPE_HANDLE_BYTES, "IPC handle size");
    HIP_TRY(hipSetDevice(db->device));
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, db->d_rec));
    memset(handle, 0, GS_STRIPE_HANDLE_BYTES);
    memcpy(handle, &h, sizeof(h));
    return GS_OK;
}

extern "C" int gs_db_stripe_attach(gs_db *db, int stripe, const void *handle) {
    if (!db || !handle) return fail(GS_E_INVALID, "NULL argument");
    if (!db->striped() || db->group) return fail(GS_E_STATE, "not a stripe of gs_db_create_stripe");
    if (stripe < 0 || stripe >= db->n_parts || stripe == db->part) return fail(GS_E_INVALID, "stripe out of range (or this handle's own)");
    if (db->present & (1u << stripe)) return fail(GS_E_STATE, "stripe already attached");
    if (db->live_runs > 0) return fail(GS_E_STATE, "the store has runs");
    HIP_TRY(hipSetDevice(db->device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    void *p = nullptr;
    HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
    db->ipc_opened.push_back(p);
    db_set_stripe(db, stripe, (const u64 *)p);
    return GS_OK;
}

// ---- a built store on the host (from the builder or from a store file) and its way into HBM
struct StoreImage {
    int k = 0, n_values = 0;
    int64_t n_entries = 0, n_stored = 0, n_in_records = 0;
    int b = 0, vbits = 0, rec_bits = 0, max_disp = 0;
    const u64 *table = nullptr;
    size_t table_words = 0;
    const u64 *gate = nullptr;
    size_t gate_words = 0;
    const uint32_t *mgate = nullptr;
    size_t mgate_words = 0;
    uint32_t mgate_ctx = 0;  // the gate is keyed by gs_gate_ctx_key
    const u64 *rec = nullptr;
    size_t rec_words = 0;
    const int32_t *parent = nullptr, *depth = nullptr, *tin = nullptr, *tout = nullptr;
};  // (table / gate / mgate / rec may lie in host memory or in a device's: store_upload copies with hipMemcpyDefault)

// one handle: the whole store (stripes <= 1), or stripe `part` of `stripes` -- the record buckets gs_stripe_first(part) up
// to gs_stripe_first(part + 1) and the table buckets gs_tab_stripe_first(..) in ONE allocation (one IPC handle), and
// everything else (gates, tree) in full
static int store_upload(const StoreImage &im, int dev_no, int stripes, int part, gs_db **res) {
    *res = nullptr;
    HIP_TRY(hipSetDevice(dev_no));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev_no));
    gs_db *db = new gs_db();
    db->device = dev_no;
    db->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const int n_values = im.n_values;
    const int64_t n_rec_total = im.rec_words ? (int64_t)1 << im.rec_bits : 0;
    int64_t rfirst = 0, rlocal = n_rec_total, tfirst = 0, tlocal = (int64_t)1 << im.b;
    if (stripes > 1) {
        rfirst = (int64_t)gs_stripe_first((uint32_t)im.rec_bits, (uint32_t)stripes, (uint32_t)part);
        rlocal = (int64_t)gs_stripe_first((uint32_t)im.rec_bits, (uint32_t)stripes, (uint32_t)part + 1) - rfirst;
        tfirst = (int64_t)gs_tab_stripe_first((uint32_t)im.b, (uint32_t)stripes, (uint32_t)part);
        tlocal = (int64_t)gs_tab_stripe_first((uint32_t)im.b, (uint32_t)stripes, (uint32_t)part + 1) - tfirst;
    }
    const size_t tbytes = (size_t)tlocal * GS_SLOTS_PER_BUCKET * sizeof(u64);
    const size_t rbytes = (size_t)rlocal * GS_REC_WORDS * sizeof(u64);
    const u64 *rsrc = im.rec + (size_t)rfirst * GS_REC_WORDS;
    const u64 *tsrc = im.table + (size_t)tfirst * GS_SLOTS_PER_BUCKET;
    hipError_t e = hipSuccess;
    if (stripes > 1) {
        e = gs_dev_alloc((void **)&db->d_rec, rbytes + tbytes);
        if (e == hipSuccess) e = hipMemcpy(db->d_rec, rsrc, rbytes, hipMemcpyDefault);
        if (e == hipSuccess) db->d_table = db->d_rec + (size_t)rlocal * GS_REC_WORDS;
    } else {
        e = gs_dev_alloc((void **)&db->d_table, tbytes);
        if (e == hipSuccess && rbytes) e = gs_dev_alloc((void **)&db->d_rec, rbytes);
        if (e == hipSuccess && rbytes) e = hipMemcpy(db->d_rec, rsrc, rbytes, hipMemcpyDefault);
    }
    if (e == hipSuccess) e = gs_dev_alloc((void **)&db->d_tree, sizeof(int32_t) * 4 * (size_t)n_values);
    if (e == hipSuccess && im.gate_words) e = gs_dev_alloc((void **)&db->d_gate, im.gate_words * sizeof(u64));
    if (e == hipSuccess && im.gate_words) e = hipMemcpy(db->d_gate, im.gate, im.gate_words * sizeof(u64), hipMemcpyDefault);
    if (e == hipSuccess && im.mgate_words) e = gs_dev_alloc((void **)&db->d_mgate, im.mgate_words * sizeof(uint32_t));
    if (e == hipSuccess && im.mgate_words) e = hipMemcpy(db->d_mgate, im.mgate, im.mgate_words * sizeof(uint32_t), hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(db->d_table, tsrc, tbytes, hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(db->d_tree, im.parent, sizeof(int32_t) * n_values, hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(db->d_tree + n_values, im.depth, sizeof(int32_t) * n_values, hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(db->d_tree + 2 * (size_t)n_values, im.tin, sizeof(int32_t) * n_values, hipMemcpyDefault);
    if (e == hipSuccess) e = hipMemcpy(db->d_tree + 3 * (size_t)n_values, im.tout, sizeof(int32_t) * n_values, hipMemcpyDefault);
    if (e != hipSuccess) {
        if (stripes > 1) db->d_table = nullptr;  // (inside d_rec)
        db_free(db);
        return hip_fail(e, "store upload");
    }
    db->info.k = im.k;
    db->info.n_values = n_values;
    db->info.n_entries = im.n_entries;
    db->info.n_stored = im.n_stored;
    db->info.n_in_records = im.n_in_records;
    db->info.rec_bytes = (int64_t)(im.rec_words * sizeof(u64));
    db->n_rec = n_rec_total;
    db->dev.rec = stripes > 1 ? nullptr : db->d_rec;
    db->dev.rec_bits = (uint32_t)im.rec_bits;
    db->info.n_buckets = (int64_t)1 << im.b;
    db->info.table_bytes = (int64_t)(im.table_words * sizeof(u64));
    db->info.max_displacement = im.max_disp;
    db->info.value_bits = im.vbits;
    db->dev.table = stripes > 1 ? nullptr : db->d_table;
    db->dev.gate = db->d_gate;
    db->dev.gate_mask = im.gate_words ? (u64)im.gate_words - 1 : 0;
    db->info.gate_bytes = (int64_t)(im.gate_words * sizeof(u64));
    db->dev.mgate = db->d_mgate;
    db->dev.mgate_bits = 0;
    while (((size_t)1 << db->dev.mgate_bits) < im.mgate_words) db->dev.mgate_bits++;
    db->dev.mgate_ctx = im.mgate_ctx;
    db->info.mgate_bytes = (int64_t)(im.mgate_words * sizeof(uint32_t));
    db->dev.bucket_bits = (uint32_t)im.b;
    db->dev.vbits = (uint32_t)im.vbits;
    db->dev.bucket_mask = (1ULL << im.b) - 1;
    db->dev.k = im.k;
    db->dev.n_values = n_values;
    db->dev.parent = db->d_tree;
    db->dev.depth = db->d_tree + n_values;
    db->dev.tin = db->d_tree + 2 * (size_t)n_values;
    db->dev.tout = db->d_tree + 3 * (size_t)n_values;
    if (stripes > 1) {
        db->n_parts = stripes;
        db->part = part;
        db->rec_first = rfirst;
        db->rec_local = rlocal;
        db->tab_first = tfirst;
        db->tab_local = tlocal;
        db->info.n_stripes = stripes;
        db->info.stripe = part;
        db->info.stripe_bytes = (int64_t)(rbytes + tbytes);
        db->dev.n_parts = (uint32_t)stripes;
        db_set_stripe(db, part, db->d_rec);
    }
    *res = db;
    return GS_OK;
}

// stripes <= 1: out[0] on `device`.  stripe_only >= 0: out[0] = that stripe on `device` (the others arrive through
// gs_db_stripe_attach).  Else every stripe in this process, out[p] on stripe_devices[p]: the handles know each other's
// stripes, which belong to all of them together.
static int store_place(const StoreImage &im, int device, int stripes, const int *stripe_devices, int stripe_only, gs_db **out) {
    if (stripes > 1 && im.rec_words == 0)
        return fail(GS_E_UNSUPPORTED, "a striped store needs super-k-mer records (k >= 19, at most 2^21 values, a non-empty store)");
    if (stripes <= 1) return store_upload(im, device, 1, 0, out);
    if (stripe_only >= 0) return store_upload(im, device, stripes, stripe_only, out);
    int rc = GS_OK;
    auto group = std::make_shared<StripeGroup>();
    std::vector<gs_db *> made;
    for (int p = 0; p < stripes && rc == GS_OK; p++) {
        gs_db *db = nullptr;
        rc = store_upload(im, stripe_devices[p], stripes, p, &db);
        if (rc == GS_OK) {
            made.push_back(db);
            group->allocs.push_back({db->device, db->d_rec});
            db->group = group;
        }
    }
    for (int p = 0; p < stripes && rc == GS_OK; p++)
        for (int q = 0; q < stripes && rc == GS_OK; q++) {
            if (q == p) continue;
            if (made[(size_t)p]->device != made[(size_t)q]->device) {
                hipSetDevice(made[(size_t)p]->device);
                int can = 0;
                hipDeviceCanAccessPeer(&can, made[(size_t)p]->device, made[(size_t)q]->device);
                if (!can)
                    rc = fail(GS_E_UNSUPPORTED, "the devices of a striped store need peer access to each other");
                else {
                    const hipError_t pe = hipDeviceEnablePeerAccess(made[(size_t)q]->device, 0);
                    if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) rc = fail(GS_E_HIP, std::string("peer access: ") + hipGetErrorString(pe));
                    (void)hipGetLastError();
                }
            }
            if (rc == GS_OK) db_set_stripe(made[(size_t)p], q, made[(size_t)q]->d_rec);
        }
    if (rc != GS_OK) {
        for (gs_db *db : made) db_free(db);
        return rc;
    }
    for (int p = 0; p < stripes; p++) out[p] = made[(size_t)p];
    return GS_OK;
}

// a zero-filled array whose pages are first touched by whoever writes them (calloc of a large block hands out untouched
// zero pages): std::vector would fill gigabytes from one thread before the parallel writers start
template <typename T>
struct Zeroed {
    T *p = nullptr;
    size_t n = 0;
    Zeroed() = default;
    Zeroed(const Zeroed &) = delete;
    Zeroed &operator=(const Zeroed &) = delete;
    size_t mapped = 0;
    ~Zeroed() { release(); }
    void release() {
        if (p) munmap(p, mapped);
        p = nullptr;
        n = mapped = 0;
    }
    void reset(size_t count) {
        release();
        if (count == 0) return;
        // anonymous mapping = untouched zero pages; transparent huge pages where the kernel grants them: the builder's
        // random accesses into gigabyte arrays (cuckoo slots, record lines, gate) otherwise miss the TLB every time
        const size_t bytes = (count * sizeof(T) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        void *m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) throw std::bad_alloc();
        madvise(m, bytes, MADV_HUGEPAGE);
        p = (T *)m;
        n = count;
        mapped = bytes;
    }
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    T *data() { return p; }
    const T *data() const { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

// [0, n) in n_thr contiguous slices, one thread each (fn(t, lo, hi)); slices do not depend on timing
template <typename F>
static void parallel_slices(int n_thr, int64_t n, F fn) {
    if (n_thr <= 1 || n < 4096) {
        fn(0, (int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < n_thr; t++) th.emplace_back([=] { fn(t, n * t / n_thr, n * (t + 1) / n_thr); });
    for (auto &x : th) x.join();
}

// GS_BUILD_TRACE=1: phase times of the host builder on stderr (developer aid)
struct BuildTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    BuildTrace() : on(getenv("GS_BUILD_TRACE") != nullptr && atoi(getenv("GS_BUILD_TRACE")) != 0), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[gs_db_create] %-28s %8.3f s\n", what, std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    }
};


// parent / depth / pre-order interval of every value index from parent_vi (-1 root, -2 no node; NULL: every value a root)
static int tree_arrays(int32_t n_values, const int32_t *parent_vi, std::vector<int32_t> &parent, std::vector<int32_t> &depth,
                       std::vector<int32_t> &tin, std::vector<int32_t> &tout) {
    parent.assign((size_t)n_values, -1);
    depth.assign((size_t)n_values, 0);
    tin.assign((size_t)n_values, 0);
    tout.assign((size_t)n_values, 0);
    for (int32_t v = 0; v < n_values; v++) {
        int32_t p = parent_vi ? parent_vi[v] : -1;
        if (p < -2 || p >= n_values || p == v) return fail(GS_E_INVALID, "parent_vi out of range");
        parent[v] = p;
    }
    std::vector<std::vector<int32_t>> kids(n_values);
    std::vector<int32_t> roots;
    for (int32_t v = 0; v < n_values; v++) {
        if (parent[v] >= 0) {
            if (parent[parent[v]] == -2) return fail(GS_E_INVALID, "parent_vi points at a value without a node");
            kids[parent[v]].push_back(v);
        } else if (parent[v] == -1)
            roots.push_back(v);
    }
    int32_t counter = 0, visited = 0;
    std::vector<std::pair<int32_t, size_t>> stack;
    for (int32_t root : roots) {
        stack.push_back({root, 0});
        tin[root] = counter++;
        depth[root] = 0;
        visited++;
        while (!stack.empty()) {
            auto &top = stack.back();
            if (top.second < kids[top.first].size()) {
                int32_t c = kids[top.first][top.second++];
                tin[c] = counter++;
                depth[c] = (int32_t)stack.size();
                visited++;
                stack.push_back({c, 0});
            } else {
                tout[top.first] = counter;
                stack.pop_back();
            }
        }
    }
    int32_t nodes = 0;
    for (int32_t v = 0; v < n_values; v++) nodes += parent[v] != -2;
    if (visited != nodes) return fail(GS_E_INVALID, "parent_vi contains a cycle");
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// the layout built on the device (gs_layout_build.hip): same rules as the host builder below
// ---------------------------------------------------------------------------------------------------
enum { GS_LB_N_E = 0, GS_LB_N_T, GS_LB_N_M, GS_LB_N_H, GS_LB_IN_REC, GS_LB_OVERFLOW, GS_LB_MAX_DISP, GS_LB_N_WIN, GS_LB_N_CTX, GS_LB_N_HINT, GS_LB_COUNTERS };

// device scratch that goes when the build is over (or fails)
struct DevPool {
    std::vector<void *> all;
    hipError_t err = hipSuccess;
    ~DevPool() {
        for (void *p : all) gs_dev_free(p);
    }
    template <typename T>
    T *get(size_t count) {
        void *p = nullptr;
        if (err == hipSuccess) err = gs_dev_alloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (err != hipSuccess) return nullptr;
        all.push_back(p);
        return (T *)p;
    }
    void drop(void *p) {
        for (void *&x : all)
            if (x == p && p) {
                gs_dev_free(p);
                x = nullptr;
            }
    }
    void *keep(void *p) {  // the pointer leaves the pool (it becomes part of the store)
        for (void *&x : all)
            if (x == p) x = nullptr;
        return p;
    }
};

// 1: built (*out), 0: this store is for the host builder (no record entries), < 0: error
// kmers / vidx: host arrays, or (on_dev) arrays in this device's memory, which are only read
static int db_create_on_device(gs_db **out, int device, int k, int64_t n, const int64_t *kmers, const int32_t *vidx, int32_t n_values,
                               const std::vector<int32_t> &parent, const std::vector<int32_t> &depth, const std::vector<int32_t> &tin,
                               const std::vector<int32_t> &tout, BuildTrace &trace, bool on_dev = false) {
    hipStream_t stream = nullptr;
    DevPool pool;
    auto bad = [&](hipError_t e, const char *what) {
        return hip_fail(e, std::string("device layout build (") + what + ")");
    };
#define LB_TRY(expr, what)                                        \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ == hipSuccess && pool.err != hipSuccess) e_ = pool.err; \
        if (e_ != hipSuccess) return bad(e_, what);               \
    } while (0)
    const size_t sn = (size_t)n;
    int64_t *d_k = on_dev ? const_cast<int64_t *>(kmers) : pool.get<int64_t>(sn);
    int32_t *d_v = on_dev ? const_cast<int32_t *>(vidx) : pool.get<int32_t>(sn);
    int32_t *d_parent = pool.get<int32_t>((size_t)n_values);
    uint32_t *e_gh = pool.get<uint32_t>(sn), *e_ohi = pool.get<uint32_t>(sn), *e_olo = pool.get<uint32_t>(sn), *e_vj = pool.get<uint32_t>(sn);
    u64 *e_sort = pool.get<u64>(sn), *e_sort2 = pool.get<u64>(sn);
    u64 *t_key = pool.get<u64>(sn);
    int32_t *t_val = pool.get<int32_t>(sn);
    uint32_t *m_gh = pool.get<uint32_t>(2 * sn), *h_gh = pool.get<uint32_t>(2 * sn);
    // context keys of the gate (gs_gate_ctx_key): collected for stores big enough to possibly need them
    int64_t ctx_min_distinct = 12000000;  // ~20 % of the 15-mer minimizer space: a filter over the minimizers alone starts to leak
    if (const char *e = getenv("GS_GATE_CTX_MIN_DISTINCT")) ctx_min_distinct = std::max<int64_t>(0, atoll(e));
    const bool ctx_possible = k >= GS_CTX_MIN_K && n >= ctx_min_distinct;
    uint32_t *h_ctx = ctx_possible ? pool.get<uint32_t>(2 * sn) : nullptr;
    u64 *cnt = pool.get<u64>(GS_LB_COUNTERS);
    LB_TRY(pool.err, "buffers");
    if (!on_dev) {
        LB_TRY(hipMemcpy(d_k, kmers, sn * sizeof(int64_t), hipMemcpyHostToDevice), "upload");
        LB_TRY(hipMemcpy(d_v, vidx, sn * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
    }
    LB_TRY(hipMemcpy(d_parent, parent.data(), (size_t)n_values * sizeof(int32_t), hipMemcpyHostToDevice), "upload");
    LB_TRY(hipMemset(cnt, 0, GS_LB_COUNTERS * sizeof(u64)), "counters");
    trace.mark("device: upload");
    LB_TRY(gs_lb_perkey(d_k, d_v, n, k, d_parent, e_gh, e_ohi, e_olo, e_vj, e_sort, e_sort2, t_key, t_val, m_gh, h_gh, h_ctx, cnt, stream), "per key");
    u64 c[GS_LB_COUNTERS];
    LB_TRY(hipMemcpy(c, cnt, sizeof(c), hipMemcpyDeviceToHost), "per key");
    if (!on_dev) {
        pool.drop(d_k);
        pool.drop(d_v);
    }
    const int64_t n_e = (int64_t)c[GS_LB_N_E], n_h = (int64_t)c[GS_LB_N_H], n_ctx = (int64_t)c[GS_LB_N_CTX];
    trace.mark("device: per key");
    if (n_e == 0) return 0;  // nothing for records: the host builder's table-only store
    // ---- entries sorted by minimizer, minimizers -> windows
    const size_t se = (size_t)n_e;
    u64 *sort_alt = pool.get<u64>(se);
    uint32_t *perm = pool.get<uint32_t>(se), *perm_alt = pool.get<uint32_t>(se);
    uint32_t *s_gh = pool.get<uint32_t>(se), *s_ohi = pool.get<uint32_t>(se), *s_olo = pool.get<uint32_t>(se), *s_vj = pool.get<uint32_t>(se);
    LB_TRY(pool.err, "sort buffers");
    LB_TRY(gs_lb_sort_entries(e_sort, e_sort2, sort_alt, perm, perm_alt, n_e, e_gh, e_ohi, e_olo, e_vj, s_gh, s_ohi, s_olo, s_vj, stream), "sort");
    pool.drop(e_sort2);
    pool.drop(e_gh);
    pool.drop(e_ohi);
    pool.drop(e_olo);
    pool.drop(e_vj);
    pool.drop(e_sort);
    pool.drop(sort_alt);
    pool.drop(perm);
    pool.drop(perm_alt);
    trace.mark("device: sort");
    uint32_t *head = pool.get<uint32_t>(se), *group = pool.get<uint32_t>(se), *g_start = pool.get<uint32_t>(se + 1);
    LB_TRY(pool.err, "group buffers");
    int64_t n_groups = 0;
    LB_TRY(gs_lb_groups(s_gh, n_e, head, group, g_start, &n_groups, stream), "groups");
    pool.drop(head);
    const size_t sw = 2 * (size_t)n_groups;
    uint8_t *assign = pool.get<uint8_t>(se);
    u64 *w_hi = pool.get<u64>(sw), *w_lo = pool.get<u64>(sw);
    uint32_t *w_valid = pool.get<uint32_t>(sw), *w_gh = pool.get<uint32_t>(sw);
    LB_TRY(pool.err, "window buffers");
    LB_TRY(gs_lb_cluster(s_gh, s_ohi, s_olo, s_vj, g_start, n_groups, k, assign, w_hi, w_lo, w_valid, w_gh, cnt, stream), "cluster");
    LB_TRY(hipMemcpy(c, cnt, sizeof(c), hipMemcpyDeviceToHost), "cluster");
    pool.drop(g_start);
    const int64_t n_win = (int64_t)c[GS_LB_N_WIN];
    trace.mark("device: cluster");
    // ---- buckets
    double rload = 0.4;
    if (const char *e = getenv("GS_REC_LOAD")) {
        const double v = atof(e);
        if (v > 0.01 && v <= 0.5) rload = v;
    }
    int rec_bits = 4;
    while (rec_bits < 29 && (double)((size_t)1 << rec_bits) * rload < (double)n_win) rec_bits++;
    const size_t n_rec = (size_t)1 << rec_bits;
    int max_rounds = 64, rounds_done = 0;
    if (const char *e = getenv("GS_REC_ROUNDS")) max_rounds = std::max(2, std::min(5000, atoi(e)));
    uint32_t *slot = pool.get<uint32_t>(n_rec), *slot2 = pool.get<uint32_t>(n_rec), *claim = pool.get<uint32_t>(n_rec);
    uint32_t *wstate = pool.get<uint32_t>(sw), *win_bucket = pool.get<uint32_t>(sw);
    u64 *d_rec = pool.get<u64>(n_rec * GS_REC_WORDS);
    LB_TRY(pool.err, "record buffers");
    LB_TRY(gs_lb_place(w_valid, w_gh, (int64_t)sw, (uint32_t)rec_bits, max_rounds, slot, slot2, claim, wstate, win_bucket, cnt + GS_LB_OVERFLOW,
                       &rounds_done, stream), "placement");
    pool.drop(wstate);
    pool.drop(slot2);
    pool.drop(claim);
    LB_TRY(gs_lb_lines(slot, (uint32_t)rec_bits, w_hi, w_lo, w_valid, s_gh, s_ohi, s_olo, s_vj, group, assign, win_bucket, n_e, k, d_rec, t_key, t_val,
                       m_gh, cnt, stream), "lines");
    LB_TRY(hipMemcpy(c, cnt, sizeof(c), hipMemcpyDeviceToHost), "lines");
    const int64_t n_t = (int64_t)c[GS_LB_N_T], n_m = (int64_t)c[GS_LB_N_M], n_in_records = (int64_t)c[GS_LB_IN_REC];
    LB_TRY(gs_lb_more(m_gh, n_m, (uint32_t)rec_bits, d_rec, stream), "more bits");
    // the windows in their second bucket (gs_mgate_hint); at most every window
    uint32_t *hint_gh = pool.get<uint32_t>(std::max<size_t>(sw, 1)), *hint_cx = pool.get<uint32_t>(std::max<size_t>(sw, 1));
    LB_TRY(pool.err, "hint buffers");
    LB_TRY(gs_lb_hint_collect(w_valid, w_gh, w_hi, w_lo, win_bucket, (int64_t)sw, (uint32_t)rec_bits, k, hint_gh, hint_cx, cnt, stream), "hints");
    LB_TRY(hipMemcpy(c, cnt, sizeof(c), hipMemcpyDeviceToHost), "hints");
    const int64_t n_hint = (int64_t)c[GS_LB_N_HINT];
    LB_TRY(hipDeviceSynchronize(), "more bits");
    for (void *p : {(void *)slot, (void *)win_bucket, (void *)assign, (void *)w_hi, (void *)w_lo, (void *)w_valid, (void *)w_gh, (void *)s_gh, (void *)s_ohi,
                    (void *)s_olo, (void *)s_vj, (void *)group, (void *)m_gh})
        pool.drop(p);
    trace.mark("device: placement + lines");
    if (trace.on)
        fprintf(stderr, "[gs_db_create] device: %lld entries, %lld minimizers, %lld windows in %lld buckets (%.3f, %d bidding rounds), %lld k-mers in records, %lld in the table\n",
                (long long)n_e, (long long)n_groups, (long long)n_win, (long long)n_rec, (double)n_win / (double)n_rec, rounds_done,
                (long long)n_in_records, (long long)n_t);
    // ---- overflow table
    const int vbits = std::max(1, bits_for((u64)n_values));
    double load = 3.0;
    if (const char *e = getenv("GS_BUCKET_LOAD")) {
        double v = atof(e);
        if (v > 0.05 && v <= 6.0) load = v;
    }
    int b = std::max(vbits + 1, 4);
    while ((double)(1ULL << b) * load < (double)n_t) b++;
    u64 *d_table = nullptr;
    int max_disp = 0;
    {
        const size_t st = (size_t)std::max<int64_t>(n_t, 1);
        u64 *rot_a = pool.get<u64>(st), *rot_b = pool.get<u64>(st);
        int32_t *val_b = pool.get<int32_t>(st), *val_c = pool.get<int32_t>(st);
        uint32_t *t_start = pool.get<uint32_t>(st), *t_left = pool.get<uint32_t>(st), *t_pos = pool.get<uint32_t>(st), *t_perm = pool.get<uint32_t>(st),
                 *t_perm2 = pool.get<uint32_t>(st);
        LB_TRY(pool.err, "table buffers");
        for (;; b++) {
            if (b > 29) return fail(GS_E_UNSUPPORTED, "store too large for 32-bit slot indices");
            uint32_t *fill_a = pool.get<uint32_t>((size_t)1 << b), *fill_b = pool.get<uint32_t>((size_t)1 << b);
            d_table = pool.get<u64>(((size_t)1 << b) * GS_SLOTS_PER_BUCKET);
            LB_TRY(pool.err, "table buffers");
            int64_t overflow = 0;
            LB_TRY(gs_lb_table(t_key, t_val, n_t, b, vbits, rot_a, rot_b, val_b, val_c, t_start, t_left, t_pos, t_perm, t_perm2, fill_a, fill_b, d_table,
                               &overflow, &max_disp, stream), "table");
            pool.drop(fill_a);
            pool.drop(fill_b);
            if (overflow == 0) break;
            pool.drop(d_table);  // a key found no slot within GS_MAX_DISP buckets: twice the buckets
        }
        for (void *p : {(void *)rot_a, (void *)rot_b, (void *)val_b, (void *)val_c, (void *)t_start, (void *)t_left, (void *)t_pos, (void *)t_perm, (void *)t_perm2}) pool.drop(p);
    }
    pool.drop(t_key);
    pool.drop(t_val);
    trace.mark("device: overflow table");
    // ---- minimizer gate
    uint32_t *h_alt = pool.get<uint32_t>((size_t)std::max<int64_t>(n_h, 1));
    LB_TRY(pool.err, "gate buffers");
    int64_t distinct = 0;
    uint32_t *h_sorted = h_gh;
    LB_TRY(gs_lb_distinct(h_gh, h_alt, n_h, cnt, &distinct, &h_sorted, stream), "distinct minimizers");
    // a store whose minimizers fill a good part of the minimizer space gets the gate keyed by minimizer + context instead
    int64_t n_gate = n_h;
    uint32_t mgate_ctx = 0;
    if (h_ctx != nullptr && distinct >= ctx_min_distinct) {
        pool.drop(h_alt);
        h_alt = pool.get<uint32_t>((size_t)std::max<int64_t>(n_ctx, 1));
        LB_TRY(pool.err, "gate buffers");
        LB_TRY(gs_lb_distinct(h_ctx, h_alt, n_ctx, cnt, &distinct, &h_sorted, stream), "distinct context keys");
        n_gate = n_ctx;
        mgate_ctx = 1;
    }
    double bits_per_min = 16.0;
    if (const char *e = getenv("GS_MGATE_BITS_PER_MIN")) bits_per_min = std::max(1.0, atof(e));
    int mgate_bits = 6;
    while (mgate_bits < 30 && (double)((size_t)32 << mgate_bits) < (double)distinct * bits_per_min) mgate_bits++;
    uint32_t *d_mgate = pool.get<uint32_t>((size_t)1 << mgate_bits);
    LB_TRY(pool.err, "gate");
    LB_TRY(gs_lb_gate(h_sorted, n_gate, (int)mgate_ctx, (uint32_t)mgate_bits, d_mgate, stream), "gate");
    LB_TRY(gs_lb_hint(hint_gh, hint_cx, n_hint, (int)mgate_ctx, (uint32_t)mgate_bits, d_mgate, stream), "gate hints");
    int32_t *d_tree = pool.get<int32_t>(4 * (size_t)n_values);
    LB_TRY(pool.err, "tree");
    LB_TRY(hipMemcpy(d_tree, parent.data(), sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice), "tree");
    LB_TRY(hipMemcpy(d_tree + n_values, depth.data(), sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice), "tree");
    LB_TRY(hipMemcpy(d_tree + 2 * (size_t)n_values, tin.data(), sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice), "tree");
    LB_TRY(hipMemcpy(d_tree + 3 * (size_t)n_values, tout.data(), sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice), "tree");
    LB_TRY(hipDeviceSynchronize(), "gate");
    trace.mark("device: gate");
#undef LB_TRY
    hipDeviceProp_t prop;
    gs_db *db = new gs_db();
    db->device = device;
    db->n_cu = (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    db->d_rec = (u64 *)pool.keep(d_rec);
    db->d_table = (u64 *)pool.keep(d_table);
    db->d_mgate = (uint32_t *)pool.keep(d_mgate);
    db->d_tree = (int32_t *)pool.keep(d_tree);
    db->n_rec = (int64_t)n_rec;
    db->info.k = k;
    db->info.n_values = n_values;
    db->info.n_entries = n;
    db->info.n_stored = n_t + n_in_records;
    db->info.n_in_records = n_in_records;
    db->info.rec_bytes = (int64_t)(n_rec * GS_REC_WORDS * sizeof(u64));
    db->info.n_buckets = (int64_t)1 << b;
    db->info.table_bytes = (int64_t)(((size_t)1 << b) * GS_SLOTS_PER_BUCKET * sizeof(u64));
    db->info.max_displacement = max_disp;
    db->info.value_bits = vbits;
    db->info.gate_bytes = 0;
    db->info.mgate_bytes = (int64_t)(((size_t)1 << mgate_bits) * sizeof(uint32_t));
    db->dev.table = db->d_table;
    db->dev.gate = nullptr;
    db->dev.gate_mask = 0;
    db->dev.mgate = db->d_mgate;
    db->dev.mgate_bits = (uint32_t)mgate_bits;
    db->dev.mgate_ctx = mgate_ctx;
    db->dev.rec = db->d_rec;
    db->dev.rec_bits = (uint32_t)rec_bits;
    db->dev.bucket_bits = (uint32_t)b;
    db->dev.vbits = (uint32_t)vbits;
    db->dev.bucket_mask = (1ULL << b) - 1;
    db->dev.k = k;
    db->dev.n_values = n_values;
    db->dev.parent = db->d_tree;
    db->dev.depth = db->d_tree + n_values;
    db->dev.tin = db->d_tree + 2 * (size_t)n_values;
    db->dev.tout = db->d_tree + 3 * (size_t)n_values;
    *out = db;
    return 1;
}

// fused: the store serves the fused kernels (gs_match_submit*, gs_match_segments) and may keep k-mers in super-k-mer
// records; a partition store (gs_db_create_part, any n_parts) keeps every key in the table, where gs_match_probe_keys looks
static int db_create_impl(gs_db **out, int device, int k, int64_t n, const int64_t *kmers, const int32_t *vidx,
                          int32_t n_values, const int32_t *parent_vi, int n_parts, int part, bool fused, int stripes,
                          const int *stripe_devices, int stripe_only) {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    for (int p = 0; p < (stripes > 1 && stripe_only < 0 ? stripes : 1); p++) out[p] = nullptr;
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (n < 0 || n_values < 1 || n_values > (1 << 24) || (n > 0 && (!kmers || !vidx)))
        return fail(GS_E_INVALID, "bad store arrays (n_values must be in [1, 2^24])");
    // GS_BUILD_DRYRUN=1 (developer aid, with GS_BUILD_TRACE): the host layout is built and timed, nothing is uploaded
    const bool dryrun = getenv("GS_BUILD_DRYRUN") != nullptr && atoi(getenv("GS_BUILD_DRYRUN")) != 0;
    int rc = dryrun ? GS_OK : use_device(device);
    if (rc) return rc;
    BuildTrace trace;
    bool ascending = true;
    for (int64_t i = 0; i < n; i++) {
        if (vidx[i] < 0 || vidx[i] >= n_values) return fail(GS_E_INVALID, "value_idx out of range");
        if (i && kmers[i] <= kmers[i - 1]) ascending = false;
        if (kmers[i] < 0 || (k < 31 && (u64)kmers[i] >> (2 * k))) return fail(GS_E_INVALID, "k-mer exceeds 2k bits");
    }
    if (!ascending) {
        // KMerStore.visit order of a RadixKMerStore (C/store/RadixKMerStore.java:714-729: by radix bucket, then by the
        // remaining bits) is not ascending.  The table does not care about the order, only that the keys are distinct.
        std::vector<int64_t> sorted(kmers, kmers + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(GS_E_INVALID, "k-mers must be distinct");
    }
    // ---- tree arrays
    std::vector<int32_t> parent, depth, tin, tout;
    rc = tree_arrays(n_values, parent_vi, parent, depth, tin, tout);
    if (rc) return rc;
    trace.mark("checks + tree");
    // ---- the layout on the device: plain fused stores with records (k >= 19, at most 2^21 values).  GS_BUILD_HOST=1 keeps
    // the host builder (the reference for the layout rules; striped / partition / table-only stores are always its job)
    {
        bool on_device = fused && n_parts == 1 && !dryrun && k >= GS_MIN_K && n_values <= GS_REC_MAX_VALUES && n > 0 && n < ((int64_t)1 << 31);
        if (const char *e = getenv("GS_BUILD_HOST")) on_device = on_device && atoi(e) == 0;
        if (const char *e = getenv("GS_MGATE")) on_device = on_device && atoi(e) != 0;
        if (const char *e = getenv("GS_RECORDS")) on_device = on_device && atoi(e) != 0;
        if (on_device && stripes <= 1) {
            const int drc = db_create_on_device(out, device, k, n, kmers, vidx, n_values, parent, depth, tin, tout, trace);
            if (drc == 1 && getenv("GS_BUILD_VERIFY") != nullptr && atoi(getenv("GS_BUILD_VERIFY")) != 0) {
                // developer aid: the image through the checks gs_db_load applies to a store file
                const int vrc = db_self_check(*out);
                if (vrc) {
                    db_free(*out);
                    *out = nullptr;
                    return vrc;
                }
            }
            if (drc != 0) return drc < 0 ? drc : GS_OK;
        } else if (on_device) {
            // a striped store: the layout on one device (the first stripe's, or this process's), the stripes cut from that
            gs_db *whole = nullptr;
            const int bdev = stripe_only >= 0 ? device : stripe_devices[0];
            HIP_TRY(hipSetDevice(bdev));
            const int drc = db_create_on_device(&whole, bdev, k, n, kmers, vidx, n_values, parent, depth, tin, tout, trace);
            if (drc < 0) return drc;
            if (drc == 1) {
                // (the stripes are copied out of the build's arrays, device to device: no host image)
                StoreImage im{};
                im.k = k;
                im.n_values = n_values;
                im.n_entries = n;
                im.n_stored = whole->info.n_stored;
                im.n_in_records = whole->info.n_in_records;
                im.b = (int)whole->dev.bucket_bits;
                im.vbits = (int)whole->dev.vbits;
                im.rec_bits = (int)whole->dev.rec_bits;
                im.max_disp = whole->info.max_displacement;
                im.table = whole->d_table;
                im.table_words = (size_t)whole->info.n_buckets * GS_SLOTS_PER_BUCKET;
                im.mgate = whole->d_mgate;
                im.mgate_words = (size_t)1 << whole->dev.mgate_bits;
                im.mgate_ctx = whole->dev.mgate_ctx;
                im.rec = whole->d_rec;
                im.rec_words = (size_t)whole->n_rec * GS_REC_WORDS;
                im.parent = parent.data();
                im.depth = depth.data();
                im.tin = tin.data();
                im.tout = tout.data();
                rc = store_place(im, device, stripes, stripe_devices, stripe_only, out);
                db_free(whole);
                trace.mark("stripes");
                return rc;
            }
        }
    }
    // ---- keys
    // Every reachable stored k-mer is looked at from both strands (gs_layout.h: gs_choose_minimizer).  If both views pick
    // the same minimizer occurrence the k-mer can live in a super-k-mer record; otherwise (and for every k-mer when the
    // store has no records) it goes to the ordinary table under its mixed key.
    struct RecEntry {
        uint32_t bucket, gh, ohi, olo, vj;  // vj = value index << 5 | offset j of the k-mer in its window
    };
    std::vector<u64> hkey;
    std::vector<int32_t> hval;
    std::vector<uint32_t> hmin;   // order hash of the minimizer(s) of every reachable key of ANY partition (k >= GS_MIN_K)
    std::vector<uint32_t> hmore;  // minimizers whose record bucket must send mismatching probes on to the table
    std::vector<uint32_t> hint_min;  // minimizers with a window in their second candidate bucket (gs_mgate_hint)
    std::vector<RecEntry> rents;
    hkey.reserve((size_t)n);
    hval.reserve((size_t)n);
    bool want_mgate = k >= GS_MIN_K;
    if (const char *e = getenv("GS_MGATE")) want_mgate = want_mgate && atoi(e) != 0;
    bool want_rec = want_mgate && fused && n_parts == 1 && n_values <= GS_REC_MAX_VALUES;
    if (const char *e = getenv("GS_RECORDS")) want_rec = want_rec && atoi(e) != 0;
    if (want_mgate) hmin.reserve((size_t)n);
    const uint32_t kmask = (1u << k) - 1u;
    {
        // per-key work (planes, representative, hash, minimizer) on all host cores: slices are converted independently
        // and concatenated in order, so the result does not depend on the thread count
        int n_thr = (int)std::min<int64_t>(std::max<unsigned>(1, std::thread::hardware_concurrency()), 32);
        if (const char *e = getenv("GS_BUILD_THREADS")) n_thr = std::max(1, std::min(64, atoi(e)));
        if (n < 200000) n_thr = 1;
        struct Slice {
            std::vector<u64> h;
            std::vector<int32_t> v;
            std::vector<uint32_t> m, more;
            std::vector<RecEntry> r;
        };
        std::vector<Slice> sl((size_t)n_thr);
        auto work = [&](int t) {
            const int64_t lo = n * t / n_thr, hi = n * (t + 1) / n_thr;
            Slice &o = sl[(size_t)t];
            if (want_rec)
                o.r.reserve((size_t)(hi - lo));
            else {
                o.h.reserve((size_t)(hi - lo));
                o.v.reserve((size_t)(hi - lo));
            }
            if (want_mgate) o.m.reserve((size_t)(hi - lo));
            for (int64_t i = lo; i < hi; i++) {
                uint32_t fhi, flo, phi, plo;
                bool reachable = java_to_planes((u64)kmers[i], k, fhi, flo);
                if (!reachable || parent[vidx[i]] == -2) continue;
                bool in_record = false;
                // the minimizer gate of a partition covers the keys of ALL partitions: the rank that encodes a read
                // (gs_match_encode) uses it to decide which k-mers are worth routing to their owner at all
                if (want_mgate) {
                    const uint32_t rhi = gs_brev32(fhi) >> (32 - k), rlo = (gs_brev32(flo) >> (32 - k)) ^ kmask;
                    uint32_t gh1, gh2, ohi1, olo1, ohi2, olo2;
                    int j1, j2;
                    // the reverse strand sees the same canonical 15-mers at mirrored offsets: one pass over the order hashes
                    // serves both views (the leftmost of equal ranks in one view is the rightmost in the other)
                    int p1 = 0, p2 = 0;
                    {
                        uint32_t best1 = 0xffffffffu, best2 = 0xffffffffu;
                        const int last = k - GS_MIN_L;
                        for (int d = 0; d <= last; d++) {
                            const uint32_t h = gs_lmer_hash((fhi >> d) & 0x7fffu, (flo >> d) & 0x7fffu);
                            const uint32_t x1 = gs_lmer_rank(h, (uint32_t)d), x2 = gs_lmer_rank(h, (uint32_t)(last - d));
                            best1 = x1 < best1 ? x1 : best1;
                            best2 = x2 < best2 ? x2 : best2;
                        }
                        p1 = (int)(best1 & 0xffu);
                        p2 = (int)(best2 & 0xffu);
                    }
                    gs_min_oriented(fhi, flo, rhi, rlo, k, p1, gh1, ohi1, olo1, j1);
                    gs_min_oriented(rhi, rlo, fhi, flo, k, p2, gh2, ohi2, olo2, j2);
                    const bool same = gh1 == gh2 && j1 == j2 && ohi1 == ohi2 && olo1 == olo2;
                    o.m.push_back(gh1);
                    if (gh2 != gh1) o.m.push_back(gh2);
                    if (want_rec) {
                        if (same) {
                            o.r.push_back(RecEntry{0u, gh1, ohi1, olo1, ((uint32_t)vidx[i] << 5) | (uint32_t)j1});
                            in_record = true;
                        } else {  // two strand views: one table slot, reachable from both record buckets
                            o.more.push_back(gh1);
                            o.more.push_back(gh2);
                        }
                    }
                }
                if (in_record) continue;
                gs_rep_planes(fhi, flo, k, kmask, phi, plo);  // the orientation the table files this k-mer under
                const u64 hk = gs_mix_planes(phi, plo);
                if (n_parts > 1 && (int)((hk >> GS_OWNER_SHIFT) % (u64)n_parts) != part) continue;  // another rank owns it
                o.h.push_back(hk);
                o.v.push_back(vidx[i]);
            }
        };
        if (n_thr == 1) {
            work(0);
        } else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(work, t);
            for (auto &x : th) x.join();
        }
        // the slices one behind the other (every thread copies its own)
        std::vector<size_t> oh((size_t)n_thr + 1, 0), om((size_t)n_thr + 1, 0), omo((size_t)n_thr + 1, 0), orr((size_t)n_thr + 1, 0);
        for (int t = 0; t < n_thr; t++) {
            oh[(size_t)t + 1] = oh[(size_t)t] + sl[(size_t)t].h.size();
            om[(size_t)t + 1] = om[(size_t)t] + sl[(size_t)t].m.size();
            omo[(size_t)t + 1] = omo[(size_t)t] + sl[(size_t)t].more.size();
            orr[(size_t)t + 1] = orr[(size_t)t] + sl[(size_t)t].r.size();
        }
        hkey.resize(oh[(size_t)n_thr]);
        hval.resize(oh[(size_t)n_thr]);
        hmin.resize(om[(size_t)n_thr]);
        hmore.resize(omo[(size_t)n_thr]);
        rents.resize(orr[(size_t)n_thr]);
        auto gather = [&](int t) {
            Slice &o = sl[(size_t)t];
            std::copy(o.h.begin(), o.h.end(), hkey.begin() + (ptrdiff_t)oh[(size_t)t]);
            std::copy(o.v.begin(), o.v.end(), hval.begin() + (ptrdiff_t)oh[(size_t)t]);
            std::copy(o.m.begin(), o.m.end(), hmin.begin() + (ptrdiff_t)om[(size_t)t]);
            std::copy(o.more.begin(), o.more.end(), hmore.begin() + (ptrdiff_t)omo[(size_t)t]);
            std::copy(o.r.begin(), o.r.end(), rents.begin() + (ptrdiff_t)orr[(size_t)t]);
            Slice().h.swap(o.h);
            std::vector<int32_t>().swap(o.v);
            std::vector<uint32_t>().swap(o.m);
            std::vector<RecEntry>().swap(o.r);
        };
        if (n_thr == 1)
            gather(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(gather, t);
            for (auto &x : th) x.join();
        }
    }
    trace.mark("per-key minimizers");
    // ---- number of DISTINCT minimizers, estimated by linear counting on a 2^26-bit sketch (a sort of the 32-bit hashes
    // costs seconds for tens of millions of keys; +-1 % is plenty for power-of-two sizes): sizes the gate and the records
    const int64_t nm = (int64_t)hmin.size();
    double distinct_min = 0;
    if (want_mgate && nm > 0) {
        const size_t sketch_bits = (size_t)1 << 26;
        std::vector<u64> sketch(sketch_bits / 64, 0);
        for (int64_t i = 0; i < nm; i++) {
            const uint32_t x = hmin[(size_t)i] * 0x9E3779B1u;  // (the hash is a bijection of the 15-mer: no extra collisions)
            sketch[(x >> 6) & (sketch.size() - 1)] |= 1ULL << (x & 63);
        }
        size_t ones = 0;
        for (u64 w : sketch) ones += (size_t)__builtin_popcountll(w);
        const double zero_frac = std::max(1e-9, 1.0 - (double)ones / (double)sketch_bits);
        distinct_min = std::min((double)nm, -(double)sketch_bits * std::log(zero_frac));
    }
    trace.mark("distinct-minimizer sketch");
    // ---- super-k-mer records (gs_layout.h): the k-mers of one minimizer are clustered into windows, every window gets one
    // of its minimizer's two buckets (cuckoo placement); the k-mers of windows that find no place join the table keys
    Zeroed<u64> rec;
    int rec_bits = 0;
    int64_t n_in_records = 0;
    if (want_rec && !rents.empty()) {
        const int64_t ne = (int64_t)rents.size();
        int n_thr = (int)std::min<int64_t>(std::max<unsigned>(1, std::thread::hardware_concurrency()), 32);
        if (const char *e = getenv("GS_BUILD_THREADS")) n_thr = std::max(1, std::min(64, atoi(e)));
        if (ne < 200000) n_thr = 1;
        // counting sort by the top bits of the minimizer hash, then every chunk is sorted and clustered on its own
        const int cbits = 8, cshift = 32 - cbits, n_chunks = 1 << cbits;
        std::vector<int64_t> cstart((size_t)n_chunks + 1, 0);
        std::vector<RecEntry> sorted((size_t)ne);
        {   // stable: thread t's entries of a chunk go behind those of the threads before it
            std::vector<std::vector<int64_t>> hist((size_t)n_thr, std::vector<int64_t>((size_t)n_chunks, 0));
            parallel_slices(n_thr, ne, [&](int t, int64_t lo, int64_t hi) {
                std::vector<int64_t> &h = hist[(size_t)t];
                for (int64_t i = lo; i < hi; i++) h[(size_t)(rents[(size_t)i].gh >> cshift)]++;
            });
            int64_t run = 0;
            for (int c = 0; c < n_chunks; c++) {
                cstart[(size_t)c] = run;
                for (int t = 0; t < n_thr; t++) {
                    const int64_t x = hist[(size_t)t][(size_t)c];
                    hist[(size_t)t][(size_t)c] = run;
                    run += x;
                }
            }
            cstart[(size_t)n_chunks] = run;
            parallel_slices(n_thr, ne, [&](int t, int64_t lo, int64_t hi) {
                std::vector<int64_t> &cur = hist[(size_t)t];
                for (int64_t i = lo; i < hi; i++) sorted[(size_t)cur[(size_t)(rents[(size_t)i].gh >> cshift)]++] = rents[(size_t)i];
            });
        }
        std::vector<RecEntry>().swap(rents);
        trace.mark("counting sort into chunks");
        struct Win {
            u64 whi, wlo, known;
            uint32_t valid, gh;
            int32_t val[17];  // offsets 0 .. k - 15 <= 16
        };
        std::vector<std::vector<Win>> chunk_wins((size_t)n_chunks);
        auto cluster_chunk = [&](int c) {
            RecEntry *lo = sorted.data() + cstart[(size_t)c], *hi = sorted.data() + cstart[(size_t)c + 1];
            std::sort(lo, hi, [](const RecEntry &a, const RecEntry &b) {
                if (a.gh != b.gh) return a.gh < b.gh;
                if ((a.vj & 31u) != (b.vj & 31u)) return (a.vj & 31u) < (b.vj & 31u);
                if (a.ohi != b.ohi) return a.ohi < b.ohi;
                return a.olo < b.olo;
            });
            std::vector<Win> &wins = chunk_wins[(size_t)c];
            for (RecEntry *g0 = lo; g0 < hi;) {  // the entries of one minimizer
                RecEntry *g1 = g0;
                while (g1 < hi && g1->gh == g0->gh) g1++;
                const size_t first = wins.size();
                for (RecEntry *e = g0; e < g1; e++) {
                    const int j = (int)(e->vj & 31u);
                    const u64 eh = (u64)e->ohi << j, el = (u64)e->olo << j, km = (u64)kmask << j;
                    size_t w = first;
                    for (; w < wins.size(); w++) {  // first window that agrees on every base both know and has offset j free
                        const Win &W = wins[w];
                        if (!((W.valid >> j) & 1u) && ((W.whi ^ eh) & W.known & km) == 0 && ((W.wlo ^ el) & W.known & km) == 0) break;
                    }
                    if (w == wins.size()) {
                        wins.push_back(Win{});
                        wins.back().gh = e->gh;
                    }
                    Win &W = wins[w];
                    W.whi |= eh;
                    W.wlo |= el;
                    W.known |= km;
                    W.valid |= 1u << j;
                    W.val[j] = (int32_t)(e->vj >> 5);
                }
                // the fullest windows of a minimizer first: only two of them can find a bucket
                std::stable_sort(wins.begin() + (ptrdiff_t)first, wins.end(),
                                 [](const Win &a, const Win &b) { return __builtin_popcount(a.valid) > __builtin_popcount(b.valid); });
                g0 = g1;
            }
        };
        if (n_thr == 1) {
            for (int c = 0; c < n_chunks; c++) cluster_chunk(c);
        } else {
            std::atomic<int> next{0};
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++)
                th.emplace_back([&] {
                    for (int c; (c = next.fetch_add(1)) < n_chunks;) cluster_chunk(c);
                });
            for (auto &x : th) x.join();
        }
        std::vector<RecEntry>().swap(sorted);
        trace.mark("sort + cluster windows");
        size_t n_win = 0;
        for (auto &v : chunk_wins) n_win += v.size();
        // windows per bucket before the bucket count doubles: with the power-of-two rounding 0.2 .. 0.4 (two-choice cuckoo
        // placement with one window per bucket works up to 0.5)
        double rload = 0.4;
        if (const char *e = getenv("GS_REC_LOAD")) {
            const double v = atof(e);
            if (v > 0.01 && v <= 0.5) rload = v;
        }
        rec_bits = 4;
        while (rec_bits < 29 && (double)((size_t)1 << rec_bits) * rload < (double)n_win) rec_bits++;
        const size_t n_rec = (size_t)1 << rec_bits;
        // cuckoo placement.  Windows are numbered in chunk order (within a minimizer: fullest first).  Two parallel rounds
        // whose outcome does not depend on timing -- every window bids for its first bucket, then the losers for their
        // second bucket among those still free, and the LOWEST number wins a bucket (atomic min) -- place ~95 % of the
        // windows; the rest goes through the sequential eviction walk.
        std::vector<const Win *> order;
        order.reserve(n_win);
        for (auto &v : chunk_wins)
            for (const Win &W0 : v) order.push_back(&W0);
        if (order.size() >= 0xffffffffull) return fail(GS_E_UNSUPPORTED, "store too large: more than 2^32 windows");
        const uint32_t EMPTY = 0xffffffffu;
        const int64_t nw = (int64_t)order.size();
        std::vector<uint32_t> slot(n_rec, EMPTY), bid;
        std::vector<uint8_t> placed((size_t)nw, 0);
        parallel_slices(n_thr, nw, [&](int, int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) {
                uint32_t *p = &slot[gs_rec_bucket(order[(size_t)i]->gh, (uint32_t)rec_bits, 0)];
                uint32_t seen = __atomic_load_n(p, __ATOMIC_RELAXED);
                while ((uint32_t)i < seen && !__atomic_compare_exchange_n(p, &seen, (uint32_t)i, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
                }
            }
        });
        parallel_slices(n_thr, nw, [&](int, int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) placed[(size_t)i] = slot[gs_rec_bucket(order[(size_t)i]->gh, (uint32_t)rec_bits, 0)] == (uint32_t)i;
        });
        bid.assign(n_rec, EMPTY);
        parallel_slices(n_thr, nw, [&](int, int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) {
                if (placed[(size_t)i]) continue;
                const uint32_t b1 = gs_rec_bucket(order[(size_t)i]->gh, (uint32_t)rec_bits, 1);
                if (slot[b1] != EMPTY) continue;  // (round 1 is over: slot is read-only here)
                uint32_t *p = &bid[b1];
                uint32_t seen = __atomic_load_n(p, __ATOMIC_RELAXED);
                while ((uint32_t)i < seen && !__atomic_compare_exchange_n(p, &seen, (uint32_t)i, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
                }
            }
        });
        parallel_slices(n_thr, (int64_t)n_rec, [&](int, int64_t lo, int64_t hi) {
            for (int64_t b = lo; b < hi; b++)
                if (bid[(size_t)b] != EMPTY) {  // (only buckets that were free after round 1 got bids)
                    slot[(size_t)b] = bid[(size_t)b];
                    placed[bid[(size_t)b]] = 1;
                }
        });
        std::vector<uint32_t>().swap(bid);
        std::vector<const Win *> homeless;
        uint64_t rng = 0x9E3779B97F4A7C15ULL;
        // A walk that has not ended after 16 evictions rarely ends at all: what blocks it is not the load but the
        // minimizers with two windows -- their two buckets are taken for good, and a window whose both buckets are such
        // (or a second pair that shares a bucket with the first) has no place whatever the walk does.  At 473 M k-mers
        // 19 % of the minimizers have two windows and 5 % more (the space of 15-mers that can BE a minimizer is only
        // ~4^15 / 2 / 9 = 60 M): 2.1 M windows are third siblings, 2.9 M walks are hopeless (the same count with 48 or 500
        // steps; 500 steps of three cache misses each made this loop a third of the build).  Those windows go to the table.
        int max_kicks = 16;
        if (const char *e = getenv("GS_REC_KICKS")) max_kicks = std::max(1, std::min(5000, atoi(e)));
        int64_t n_walks = 0, n_kicks = 0, n_sib_first = 0, n_sib_later = 0, n_exhausted = 0;
        for (int64_t wi = 0; wi < nw; wi++) {
            if (placed[(size_t)wi]) continue;
            n_walks++;
            uint32_t cur = (uint32_t)wi;
            uint32_t at = gs_rec_bucket(order[cur]->gh, (uint32_t)rec_bits, 0);
            for (int kick = 0; cur != EMPTY && kick < max_kicks; kick++) {
                n_kicks++;
                const uint32_t gh = order[cur]->gh;
                const uint32_t b0 = gs_rec_bucket(gh, (uint32_t)rec_bits, 0), b1 = gs_rec_bucket(gh, (uint32_t)rec_bits, 1);
                if (slot[b0] == EMPTY) {
                    slot[b0] = cur;
                    cur = EMPTY;
                } else if (slot[b1] == EMPTY) {
                    slot[b1] = cur;
                    cur = EMPTY;
                } else {  // both taken: evict one of them (not the bucket we just came from) and carry it on
                    const bool sib0 = order[slot[b0]]->gh == gh, sib1 = order[slot[b1]]->gh == gh;
                    if (sib0 && sib1) {  // its own sibling windows hold both buckets: no place for a third
                        (kick == 0 ? n_sib_first : n_sib_later)++;
                        break;
                    }
                    rng = rng * 6364136223846793005ULL + 1442695040888963407ULL;
                    uint32_t victim = (rng >> 40) & 1 ? b1 : b0;
                    if (kick > 0 && victim == at && b0 != b1) victim = victim == b0 ? b1 : b0;
                    if (order[slot[victim]]->gh == gh) victim = victim == b0 ? b1 : b0;  // (fuller siblings stay)
                    std::swap(cur, slot[victim]);
                    at = victim;
                    if (kick == max_kicks - 1) n_exhausted++;
                }
            }
            if (cur != EMPTY) homeless.push_back(order[cur]);
        }
        std::vector<uint8_t>().swap(placed);
        if (trace.on) {
            int64_t hist[5] = {0, 0, 0, 0, 0}, wsum[5] = {0, 0, 0, 0, 0};
            for (int64_t i = 0; i < nw;) {
                int64_t j = i;
                while (j < nw && order[(size_t)j]->gh == order[(size_t)i]->gh) j++;
                const int64_t c = j - i, slot_no = c >= 17 ? 4 : c >= 3 ? 3 : c;
                hist[slot_no]++;
                wsum[slot_no] += c;
                i = j;
            }
            fprintf(stderr, "[gs_db_create] minimizers with 1 / 2 / 3..16 / 17+ windows: %lld / %lld / %lld / %lld (windows: %lld / %lld / %lld / %lld)\n",
                    (long long)hist[1], (long long)hist[2], (long long)hist[3], (long long)hist[4], (long long)wsum[1], (long long)wsum[2],
                    (long long)wsum[3], (long long)wsum[4]);
        }
        if (trace.on)
            fprintf(stderr, "[gs_db_create] %lld windows in %lld buckets (%.3f), %lld walks, %lld steps, %lld windows to the table (third sibling at once %lld, later %lld, walk given up %lld)\n",
                    (long long)nw, (long long)n_rec, (double)nw / (double)n_rec, (long long)n_walks, (long long)n_kicks, (long long)homeless.size(),
                    (long long)n_sib_first, (long long)n_sib_later, (long long)n_exhausted);
        trace.mark("cuckoo placement");
        rec.reset(n_rec * GS_REC_WORDS);
        {
            std::vector<int64_t> cnt((size_t)n_thr, 0);
            std::vector<std::vector<uint32_t>> hint_of((size_t)n_thr);
            parallel_slices(n_thr, (int64_t)n_rec, [&](int t, int64_t lo, int64_t hi) {
                int64_t mine = 0;
                for (int64_t b = lo; b < hi; b++) {
                    if (b + 8 < hi && slot[(size_t)b + 8] != EMPTY) __builtin_prefetch(order[slot[(size_t)b + 8]]);
                    if (slot[(size_t)b] == EMPTY) continue;
                    const Win *W = order[slot[(size_t)b]];
                    if ((uint32_t)b != gs_rec_bucket(W->gh, (uint32_t)rec_bits, 0)) hint_of[(size_t)t].push_back(W->gh);  // gs_mgate_hint
                    u64 *rp = rec.data() + (size_t)b * GS_REC_WORDS;
                    rp[0] = W->whi;
                    rp[1] = W->wlo | ((u64)W->valid << GS_REC_WIN_BITS);
                    for (uint32_t m = W->valid; m; m &= m - 1) {
                        const int j = __builtin_ctz(m);
                        rp[2 + j / 3] |= (u64)W->val[j] << (GS_REC_VAL_BITS * (j % 3));
                        mine++;
                    }
                }
                cnt[(size_t)t] = mine;
            });
            for (int64_t x : cnt) n_in_records += x;
            for (const auto &h : hint_of) hint_min.insert(hint_min.end(), h.begin(), h.end());
        }
        for (const Win *W : homeless) {  // their k-mers become table keys, reachable through both buckets' `more` bit
            for (uint32_t m = W->valid; m; m &= m - 1) {
                const int j = __builtin_ctz(m);
                uint32_t phi, plo;
                gs_rep_planes((uint32_t)(W->whi >> j) & kmask, (uint32_t)(W->wlo >> j) & kmask, k, kmask, phi, plo);
                hkey.push_back(gs_mix_planes(phi, plo));
                hval.push_back(W->val[j]);
            }
            hmore.push_back(W->gh);
        }
        // the `more` bit of both buckets of these minimizers (OR is order-free: threads + atomics give the same lines)
        parallel_slices(n_thr, (int64_t)hmore.size(), [&](int, int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++)
                for (int ch = 0; ch < 2; ch++) {
                    u64 *rp = rec.data() + (size_t)gs_rec_bucket(hmore[(size_t)i], (uint32_t)rec_bits, ch) * GS_REC_WORDS;
                    if (__atomic_load_n(&rp[2], __ATOMIC_RELAXED) & GS_REC_MORE) continue;  // (set by an earlier entry: every word of the line has it then, or will)
                    for (int x = 2; x < GS_REC_WORDS; x++) __atomic_fetch_or(&rp[x], GS_REC_MORE, __ATOMIC_RELAXED);
                }
        });
        trace.mark("record lines + more bits");
    }  // (no eligible k-mer at all: no records, every key is in the table and the kernels take the table path)
    const int64_t ns = (int64_t)hkey.size();
    const int vbits = std::max(1, bits_for((u64)n_values));
    // keys per 8-slot bucket before the bucket count doubles: with the power-of-two rounding the table ends up at
    // 1.5 .. 3 keys per bucket.  Measured on a 47 M-k-mer store: 2.8 keys/bucket (1 GiB) is 5 % faster than 1.4 (2 GiB).
    double load = 3.0;
    if (const char *e = getenv("GS_BUCKET_LOAD")) {
        double v = atof(e);
        if (v > 0.05 && v <= 6.0) load = v;
    }
    int b = std::max(vbits + 1, stripes > 1 ? 5 : 4);  // slot bits: (62-b) rem + 2 disp + vbits value + 1 seen <= 64
    while ((double)(1ULL << b) * load < (double)ns) b++;
    std::vector<u64> table;
    int max_disp = 0;
    for (;; b++) {
        if (b > 29) return fail(GS_E_UNSUPPORTED, "store too large for 32-bit slot indices");
        const u64 nb = 1ULL << b, mask = nb - 1;
        table.assign((size_t)nb * GS_SLOTS_PER_BUCKET, 0);
        std::vector<uint8_t> fill((size_t)nb, 0);
        bool ok = true;
        max_disp = 0;
        for (int64_t i = 0; i < ns && ok; i++) {
            const u64 h = hkey[i], home = h & mask, rem = h >> b;
            int d = 0;
            for (; d <= GS_MAX_DISP; d++) {
                const u64 bk = (home + d) & mask;
                if (fill[bk] < GS_SLOTS_PER_BUCKET) {
                    table[bk * GS_SLOTS_PER_BUCKET + fill[bk]++] =
                        (rem << (vbits + 3)) | ((u64)d << (vbits + 1)) | ((u64)(hval[i] + 1) << 1);
                    break;
                }
            }
            if (d > GS_MAX_DISP) ok = false;
            max_disp = std::max(max_disp, d);
        }
        if (ok) break;
    }
    trace.mark("overflow table");
    // ---- L2-resident gate (see gs_layout.h): ~8-16 bits per key, only if it fits the per-XCD L2 budget
    std::vector<u64> gate;
    {
        size_t max_bytes = (size_t)2 << 20;
        if (const char *e = getenv("GS_GATE_MAX_BYTES")) max_bytes = (size_t)atoll(e);
        size_t bits_per_key = 8;  // rounded up to a power-of-two word count: 8..16 bits per key
        if (const char *e = getenv("GS_GATE_BITS_PER_KEY")) bits_per_key = (size_t)std::max(1, atoi(e));
        int wbits = 3;
        while (((size_t)64 << wbits) < (size_t)ns * bits_per_key) wbits++;
        if (ns > 0 && ((size_t)8 << wbits) <= max_bytes && b + wbits <= GS_GATE_FIELD_SHIFT) {
            gate.assign((size_t)1 << wbits, 0);
            const u64 gmask = ((u64)1 << wbits) - 1;
            for (int64_t i = 0; i < ns; i++) gate[(hkey[i] >> b) & gmask] |= gs_gate_bits(hkey[i]);
        }
    }
    // ---- minimizer gate (gs_layout.h): 16-32 bits per DISTINCT minimizer, 2 bits set per entry, 32-bit words
    Zeroed<uint32_t> mgate;
    int mgate_bits = 0;
    if (want_mgate && nm > 0) {
        const double distinct = distinct_min;
        double bits_per_min = 16.0;  // rounded up to a power-of-two word count: 16..32 bits per distinct minimizer
        if (const char *e = getenv("GS_MGATE_BITS_PER_MIN")) bits_per_min = std::max(1.0, atof(e));
        mgate_bits = 6;
        while (mgate_bits < 30 && (double)((size_t)32 << mgate_bits) < distinct * bits_per_min) mgate_bits++;
        mgate.reset((size_t)1 << mgate_bits);
        int g_thr = (int)std::min<int64_t>(std::max<unsigned>(1, std::thread::hardware_concurrency()), 32);
        if (const char *e = getenv("GS_BUILD_THREADS")) g_thr = std::max(1, std::min(64, atoi(e)));
        parallel_slices(nm < 200000 ? 1 : g_thr, nm, [&](int, int64_t lo, int64_t hi) {  // (OR is order-free)
            for (int64_t i = lo; i < hi; i++) {
                uint32_t *w = mgate.data() + gs_mgate_word(hmin[(size_t)i], (uint32_t)mgate_bits);
                const uint32_t bits = gs_mgate_bits(hmin[(size_t)i]);
                if ((__atomic_load_n(w, __ATOMIC_RELAXED) & bits) != bits) __atomic_fetch_or(w, bits, __ATOMIC_RELAXED);
            }
        });
        for (uint32_t h : hint_min) mgate.data()[gs_mgate_word(h, (uint32_t)mgate_bits)] |= gs_mgate_hint(h);  // windows in their second bucket
    }
    trace.mark("gates");
    StoreImage im{};
    im.k = k;
    im.n_values = n_values;
    im.n_entries = n;
    im.n_stored = ns + n_in_records;
    im.n_in_records = n_in_records;
    im.b = b;
    im.vbits = vbits;
    im.rec_bits = rec_bits;
    im.max_disp = max_disp;
    im.table = table.data();
    im.table_words = table.size();
    im.gate = gate.data();
    im.gate_words = gate.size();
    im.mgate = mgate.data();
    im.mgate_words = mgate.size();
    im.rec = rec.data();
    im.rec_words = rec.size();
    im.parent = parent.data();
    im.depth = depth.data();
    im.tin = tin.data();
    im.tout = tout.data();
    if (dryrun) return fail(GS_E_UNSUPPORTED, "GS_BUILD_DRYRUN: layout built, nothing uploaded");
    rc = store_place(im, device, stripes, stripe_devices, stripe_only, out);
    trace.mark("upload");
    return rc;
}

extern "C" int gs_db_get_info(const gs_db *db, gs_db_info *info) {
    if (!db || !info) return fail(GS_E_INVALID, "NULL argument");
    *info = db->info;
    return GS_OK;
}

// ---- native store file: the built device image (table, gate, tree) so that a later process skips the rebuild.
// Layout: GsStoreFileHeader | table (n_buckets*8 u64) | gate (gate_bytes) | tree (4*n_values int32)
struct GsStoreFileHeader {
    char magic[8];  // "GSSTORE9"
    gs_db_info info;
    uint32_t bucket_bits, vbits;  // (bit 31 of vbits: the minimizer gate is keyed by gs_gate_ctx_key, GsDbDev::mgate_ctx)
    uint64_t gate_words;
    uint64_t mgate_words;  // 32-bit words, a power of two
    uint64_t rec_buckets;  // super-k-mer record buckets (GS_REC_WORDS words each), a power of two or 0
    uint64_t checksum;     // StoreChecksum (gs_checksum.h) over table | gate | mgate | records | tree
};

// what the kernels index with: every field of a store image that came from a file is checked before it reaches HBM
template <typename Words>
static const char *store_image_defect(const GsStoreFileHeader &h, const Words &table, const Words &rec, const std::vector<int32_t> &tree) {
    const gs_db_info &in = h.info;
    if (in.k < 1 || in.k > 31) return "k outside [1, 31]";
    if (in.n_values < 1 || in.n_values > (1 << 24)) return "n_values outside [1, 2^24]";
    if (h.vbits < 1 || h.vbits > 25 || ((u64)in.n_values >> h.vbits) != 0) return "value bits do not hold n_values";
    if ((int)h.bucket_bits < std::max((int)h.vbits + 1, 4) || h.bucket_bits > 29) return "bucket bits out of range";
    if (in.n_buckets != ((int64_t)1 << h.bucket_bits) || in.table_bytes != in.n_buckets * 64) return "table size does not match the bucket count";
    if (in.value_bits != (int32_t)h.vbits) return "value bits disagree";
    if ((h.gate_words & (h.gate_words - 1)) != 0 || h.gate_words > ((uint64_t)1 << 28)) return "gate size is not a power of two";
    if (h.gate_words && h.bucket_bits + (uint32_t)bits_for(h.gate_words - 1) > GS_GATE_FIELD_SHIFT) return "gate too large for its index field";
    if ((h.mgate_words & (h.mgate_words - 1)) != 0 || h.mgate_words > ((uint64_t)1 << 30)) return "minimizer gate size is not a power of two";
    if (h.mgate_words && in.k < GS_MIN_K) return "minimizer gate on a store with k < 19";
    if (in.gate_bytes != (int64_t)(h.gate_words * 8) || in.mgate_bytes != (int64_t)(h.mgate_words * 4)) return "gate sizes disagree";
    if ((h.rec_buckets & (h.rec_buckets - 1)) != 0 || h.rec_buckets > ((uint64_t)1 << 29) || (h.rec_buckets && !h.mgate_words)) return "record bucket count is not a power of two";
    if (in.rec_bytes != (int64_t)(h.rec_buckets * GS_REC_WORDS * 8)) return "record size disagrees";
    if (h.rec_buckets && in.n_values > GS_REC_MAX_VALUES) return "records on a store with more than 2^21 values";
    if (in.max_displacement < 0 || in.max_displacement > GS_MAX_DISP) return "displacement out of range";
    const int32_t nv = in.n_values;
    const int32_t *parent = tree.data(), *depth = parent + nv, *tin = depth + nv, *tout = tin + nv;
    for (int32_t v = 0; v < nv; v++) {
        if (parent[v] < -2 || parent[v] >= nv || parent[v] == v) return "tree: parent out of range";
        if (parent[v] == -2) continue;
        if (tin[v] < 0 || tout[v] <= tin[v] || tout[v] > nv || depth[v] < 0 || depth[v] >= nv) return "tree: pre-order interval out of range";
        if (parent[v] >= 0) {  // a child's interval nests strictly inside its parent's, one level down: walks end at a root
            const int32_t p = parent[v];
            if (parent[p] == -2 || depth[v] != depth[p] + 1 || tin[v] <= tin[p] || tout[v] > tout[p]) return "tree: child interval not nested in its parent's";
        } else if (depth[v] != 0)
            return "tree: root with a depth";
    }
    // the slots and the record lines on all cores (slices; the first defect of the lowest slice is reported)
    const u64 vmask = ((u64)1 << h.vbits) - 1;
    const int c_off = in.k - GS_MIN_L;
    const size_t n_lines = rec.size() / GS_REC_WORDS;
    const int n_thr = (table.size() + rec.size()) < ((size_t)1 << 22) ? 1 : (int)std::min<unsigned>(32, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    std::vector<int64_t> c_stored((size_t)n_thr, 0), c_rec((size_t)n_thr, 0);
    std::vector<const char *> why((size_t)n_thr, nullptr);
    auto part = [&](int t) {
        const char *bad = nullptr;
        int64_t st = 0, ir = 0;
        for (size_t i = table.size() * (size_t)t / (size_t)n_thr, e = table.size() * ((size_t)t + 1) / (size_t)n_thr; i < e && !bad; i++) {
            const u64 s = table[i];
            if (s == 0) continue;
            const u64 v1 = (s >> 1) & vmask;
            if (v1 == 0 || v1 > (u64)nv || parent[v1 - 1] == -2) bad = "table: slot value without a tree node";
            else if (s & 1) bad = "table: seen bit set in a stored image";
            st++;
        }
        for (size_t b = n_lines * (size_t)t / (size_t)n_thr, e = n_lines * ((size_t)t + 1) / (size_t)n_thr; b < e && !bad; b++) {
            const u64 *rp = rec.data() + b * GS_REC_WORDS;
            if (rp[0] >> GS_REC_WIN_BITS) bad = "records: seen bit set in a stored image";
            uint32_t valid = (uint32_t)(rp[1] >> GS_REC_WIN_BITS);
            if (!bad && (valid >> (c_off + 1))) bad = "records: k-mer offset beyond the window";
            for (; valid && !bad; valid &= valid - 1) {
                const int j = __builtin_ctz(valid);
                const u64 vi = (rp[2 + j / 3] >> (GS_REC_VAL_BITS * (j % 3))) & (GS_REC_MAX_VALUES - 1);
                if (vi >= (u64)nv || parent[vi] == -2) bad = "records: value without a tree node";
                ir++;
            }
        }
        c_stored[(size_t)t] = st;
        c_rec[(size_t)t] = ir;
        why[(size_t)t] = bad;
    };
    if (n_thr == 1)
        part(0);
    else {
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; t++) th.emplace_back(part, t);
        for (auto &x : th) x.join();
    }
    int64_t stored = 0, in_records = 0;
    for (int t = 0; t < n_thr; t++) {
        if (why[(size_t)t]) return why[(size_t)t];
        stored += c_stored[(size_t)t];
        in_records += c_rec[(size_t)t];
    }
    if (in_records != in.n_in_records) return "records: entry count disagrees with the header";
    if (stored + in_records != in.n_stored) return "table: entry count disagrees with the header";
    return nullptr;
}

// the store's image back to the host and through store_image_defect (GS_BUILD_VERIFY=1: after every device build)
static int db_self_check(gs_db *db) {
    GsStoreFileHeader h{};
    h.info = db->info;
    h.bucket_bits = db->dev.bucket_bits;
    h.vbits = db->dev.vbits;
    h.gate_words = db->d_gate ? db->dev.gate_mask + 1 : 0;
    h.mgate_words = db->d_mgate ? (uint64_t)1 << db->dev.mgate_bits : 0;
    h.rec_buckets = (uint64_t)db->n_rec;
    const size_t nv = (size_t)db->info.n_values;
    Zeroed<u64> table, rec;
    table.reset((size_t)db->info.n_buckets * GS_SLOTS_PER_BUCKET);
    rec.reset((size_t)h.rec_buckets * GS_REC_WORDS);
    std::vector<int32_t> tree(4 * nv);
    HIP_TRY(hipMemcpy(table.data(), db->d_table, table.size() * sizeof(u64), hipMemcpyDeviceToHost));
    if (!rec.empty()) HIP_TRY(hipMemcpy(rec.data(), db->d_rec, rec.size() * sizeof(u64), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tree.data(), db->d_tree, tree.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (const char *why = store_image_defect(h, table, rec, tree)) return fail(GS_E_HIP, std::string("GS_BUILD_VERIFY: the device-built store fails the image checks: ") + why);
    if (db->info.n_stored > db->info.n_entries) return fail(GS_E_HIP, "GS_BUILD_VERIFY: more k-mers stored than handed in");
    return GS_OK;
}

extern "C" int gs_db_save(gs_db *db, const char *path) try {
    if (!db || !path) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(db->device));
    if (db->unique_owner) return fail(GS_E_STATE, "a unique-counting run is active on this store (seen bits are set)");
    if (db->striped()) return fail(GS_E_UNSUPPORTED, "a striped store is not saved as such: save the store built by gs_db_create");
    GsStoreFileHeader h{};
    memcpy(h.magic, "GSSTORE9", 8);
    h.info = db->info;
    h.bucket_bits = db->dev.bucket_bits;
    h.vbits = db->dev.vbits;
    h.gate_words = db->d_gate ? db->dev.gate_mask + 1 : 0;
    h.mgate_words = db->d_mgate ? (uint64_t)1 << db->dev.mgate_bits : 0;
    h.rec_buckets = (uint64_t)db->n_rec;
    const size_t nv = (size_t)db->info.n_values;
    Zeroed<u64> table, rec;  // (untouched pages: the copy from the device is the first to touch them)
    table.reset((size_t)db->info.n_buckets * GS_SLOTS_PER_BUCKET);
    rec.reset((size_t)h.rec_buckets * GS_REC_WORDS);
    std::vector<u64> gate((size_t)h.gate_words);
    if (!rec.empty()) HIP_TRY(hipMemcpy(rec.data(), db->d_rec, rec.size() * sizeof(u64), hipMemcpyDeviceToHost));
    std::vector<uint32_t> mgate((size_t)h.mgate_words);
    std::vector<int32_t> tree(4 * nv);
    HIP_TRY(hipMemcpy(table.data(), db->d_table, table.size() * sizeof(u64), hipMemcpyDeviceToHost));
    if (!gate.empty()) HIP_TRY(hipMemcpy(gate.data(), db->d_gate, gate.size() * sizeof(u64), hipMemcpyDeviceToHost));
    if (!mgate.empty()) HIP_TRY(hipMemcpy(mgate.data(), db->d_mgate, mgate.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tree.data(), db->d_tree, tree.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    {
        StoreChecksum cs;
        cs.add(table.data(), table.size() * sizeof(u64));
        cs.add(gate.data(), gate.size() * sizeof(u64));
        cs.add(mgate.data(), mgate.size() * sizeof(uint32_t));
        cs.add(rec.data(), rec.size() * sizeof(u64));
        cs.add(tree.data(), tree.size() * sizeof(int32_t));
        h.checksum = cs.value();
    }
    FILE *f = fopen(path, "wb");
    if (!f) return fail(GS_E_IO, std::string("cannot open ") + path);
    if (db->dev.mgate_ctx) h.vbits |= 0x80000000u;  // (the flag travels in bit 31 of the header's vbits word)
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && fflush(f) == 0;
    // the payload with several threads (pwrite), as gs_db_load reads it
    const int fd = fileno(f);
    off_t at = (off_t)sizeof(h);
    auto par_write = [&](const void *src, size_t bytes) {
        const int n_thr = bytes < ((size_t)64 << 20) ? 1 : (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
        std::atomic<bool> good{true};
        auto part = [&](int t) {
            size_t lo = bytes * (size_t)t / (size_t)n_thr;
            const size_t hi = bytes * ((size_t)t + 1) / (size_t)n_thr;
            while (lo < hi) {
                const ssize_t r = pwrite(fd, (const char *)src + lo, std::min<size_t>(hi - lo, (size_t)1 << 30), at + (off_t)lo);
                if (r <= 0) {
                    good = false;
                    return;
                }
                lo += (size_t)r;
            }
        };
        if (n_thr == 1)
            part(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(part, t);
            for (auto &x : th) x.join();
        }
        at += (off_t)bytes;
        return good.load();
    };
    ok = ok && par_write(table.data(), table.size() * sizeof(u64)) && par_write(gate.data(), gate.size() * sizeof(u64)) &&
         par_write(mgate.data(), mgate.size() * sizeof(uint32_t)) && par_write(rec.data(), rec.size() * sizeof(u64)) &&
         par_write(tree.data(), tree.size() * sizeof(int32_t));
    ok = (fclose(f) == 0) && ok;
    return ok ? GS_OK : fail(GS_E_IO, std::string("short write to ") + path);
}
GS_API_CATCH

// a store file into HBM: whole (stripes <= 1) or striped, as store_place
static int db_load_impl(gs_db **out, int device, const char *path, int stripes, const int *stripe_devices, int stripe_only) {
    if (!out || !path) return fail(GS_E_INVALID, "NULL argument");
    for (int p = 0; p < (stripes > 1 && stripe_only < 0 ? stripes : 1); p++) out[p] = nullptr;
    int rc = use_device(device);
    if (rc) return rc;
    FILE *f = fopen(path, "rb");
    if (!f) return fail(GS_E_INVALID, std::string("cannot open ") + path);
    GsStoreFileHeader h{};
    uint32_t file_mgate_ctx = 0;
    const bool got_header = fread(&h, sizeof(h), 1, f) == 1;
    if (got_header) {
        file_mgate_ctx = h.vbits >> 31;
        h.vbits &= 0x7fffffffu;
    }
    if (!got_header || memcmp(h.magic, "GSSTORE9", 8) != 0 || h.info.n_values < 1 || h.info.n_values > (1 << 24) ||
        h.bucket_bits > 29 || h.info.n_buckets != ((int64_t)1 << h.bucket_bits) || h.vbits > 25 ||
        h.gate_words > ((uint64_t)1 << 28) || h.mgate_words > ((uint64_t)1 << 30) || h.rec_buckets > ((uint64_t)1 << 29)) {
        fclose(f);
        return fail(GS_E_INVALID, std::string(path) + " is not a gsgpu store file (or one of another layout version)");
    }
    const size_t nv = (size_t)h.info.n_values;
    {   // the payload the header announces must be exactly what the file holds
        const uint64_t want = (uint64_t)sizeof(h) + (uint64_t)h.info.n_buckets * 64 + h.gate_words * 8 + h.mgate_words * 4 + h.rec_buckets * GS_REC_WORDS * 8 + (uint64_t)nv * 16;
        if (fseeko(f, 0, SEEK_END) != 0 || (uint64_t)ftello(f) != want || fseeko(f, (off_t)sizeof(h), SEEK_SET) != 0) {
            fclose(f);
            return fail(GS_E_INVALID, std::string(path) + ": file size does not match its header (truncated or damaged)");
        }
    }
    // (the big arrays as untouched pages: the reading threads are the first to touch them)
    Zeroed<u64> table, rec;
    table.reset((size_t)h.info.n_buckets * GS_SLOTS_PER_BUCKET);
    rec.reset((size_t)h.rec_buckets * GS_REC_WORDS);
    std::vector<u64> gate((size_t)h.gate_words);
    std::vector<uint32_t> mgate((size_t)h.mgate_words);
    std::vector<int32_t> tree(4 * nv);
    // the payload with several threads (pread): one thread copies a page-cached file at 2-3 GB/s, a big store has 10 GB
    const int fd = fileno(f);
    off_t at = (off_t)sizeof(h);
    auto par_read = [&](void *dst, size_t bytes) {
        const int n_thr = bytes < ((size_t)64 << 20) ? 1 : (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
        std::atomic<bool> good{true};
        auto part = [&](int t) {
            size_t lo = bytes * (size_t)t / (size_t)n_thr;
            const size_t hi = bytes * ((size_t)t + 1) / (size_t)n_thr;
            while (lo < hi) {
                const ssize_t r = pread(fd, (char *)dst + lo, std::min<size_t>(hi - lo, (size_t)1 << 30), at + (off_t)lo);
                if (r <= 0) {
                    good = false;
                    return;
                }
                lo += (size_t)r;
            }
        };
        if (n_thr == 1)
            part(0);
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < n_thr; t++) th.emplace_back(part, t);
            for (auto &x : th) x.join();
        }
        at += (off_t)bytes;
        return good.load();
    };
    const bool ok = par_read(table.data(), table.size() * sizeof(u64)) && par_read(gate.data(), gate.size() * sizeof(u64)) &&
                    par_read(mgate.data(), mgate.size() * sizeof(uint32_t)) && par_read(rec.data(), rec.size() * sizeof(u64)) &&
                    par_read(tree.data(), tree.size() * sizeof(int32_t));
    fclose(f);
    if (!ok) return fail(GS_E_INVALID, std::string(path) + " is truncated");
    {
        StoreChecksum cs;
        cs.add(table.data(), table.size() * sizeof(u64));
        cs.add(gate.data(), gate.size() * sizeof(u64));
        cs.add(mgate.data(), mgate.size() * sizeof(uint32_t));
        cs.add(rec.data(), rec.size() * sizeof(u64));
        cs.add(tree.data(), tree.size() * sizeof(int32_t));
        if (cs.value() != h.checksum) return fail(GS_E_INVALID, std::string(path) + ": payload checksum mismatch (damaged file)");
    }
    if (const char *why = store_image_defect(h, table, rec, tree)) return fail(GS_E_INVALID, std::string(path) + ": " + why);
    StoreImage im{};
    im.k = h.info.k;
    im.n_values = h.info.n_values;
    im.n_entries = h.info.n_entries;
    im.n_stored = h.info.n_stored;
    im.n_in_records = h.info.n_in_records;
    im.b = (int)h.bucket_bits;
    im.vbits = (int)h.vbits;
    im.rec_bits = 0;
    while (((uint64_t)1 << im.rec_bits) < h.rec_buckets) im.rec_bits++;
    im.max_disp = h.info.max_displacement;
    im.table = table.data();
    im.table_words = table.size();
    im.gate = gate.data();
    im.gate_words = gate.size();
    im.mgate = mgate.data();
    im.mgate_words = mgate.size();
    im.mgate_ctx = (file_mgate_ctx && h.info.k >= GS_CTX_MIN_K && !mgate.empty()) ? 1u : 0u;
    im.rec = rec.data();
    im.rec_words = rec.size();
    im.parent = tree.data();
    im.depth = tree.data() + nv;
    im.tin = tree.data() + 2 * nv;
    im.tout = tree.data() + 3 * nv;
    return store_place(im, device, stripes, stripe_devices, stripe_only, out);
}

extern "C" int gs_db_load(gs_db **out, int device, const char *path) try {
    return db_load_impl(out, device, path, 1, nullptr, -1);
}
GS_API_CATCH

extern "C" int gs_db_load_striped(gs_db **out, const int *devices, int n_stripes, const char *path) try {
    if (!out || !devices || n_stripes < 2 || n_stripes > GS_MAX_STRIPES) return fail(GS_E_INVALID, "a striped store spans 2..8 devices");
    for (int p = 0; p < n_stripes; p++) {
        out[p] = nullptr;
        const int rc = use_device(devices[p]);
        if (rc) return rc;
    }
    return db_load_impl(out, devices[0], path, n_stripes, devices, -1);
}
GS_API_CATCH

extern "C" int gs_db_load_stripe(gs_db **out, int device, int n_stripes, int stripe, const char *path) try {
    if (!out || n_stripes < 2 || n_stripes > GS_MAX_STRIPES || stripe < 0 || stripe >= n_stripes)
        return fail(GS_E_INVALID, "a striped store spans 2..8 devices");
    return db_load_impl(out, device, path, n_stripes, nullptr, stripe);
}
GS_API_CATCH

extern "C" int gs_db_destroy(gs_db *db) {
    if (!db) return GS_OK;
    if (db->live_runs > 0) {  // freed by the last gs_match_destroy
        db->destroy_pending = true;
        return GS_OK;
    }
    db_free(db);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// the store read back (gs_export.hip): KMerStore.visit, Database.getStats, KMerFastqGenerator
// ---------------------------------------------------------------------------------------------------
// the part of the store this handle holds: all of it, a partition's table, or a stripe's record lines + table buckets
static GsExportParams export_params(const gs_db *db, int32_t sel_vi, int with_desc) {
    GsExportParams P{};
    P.rec = db->d_rec;
    P.n_rec = db->striped() ? db->rec_local : (db->d_rec ? db->n_rec : 0);
    P.tab = db->d_table;
    P.tab_first = db->striped() ? db->tab_first : 0;
    P.n_tab = db->striped() ? db->tab_local : db->info.n_buckets;
    P.bucket_bits = db->dev.bucket_bits;
    P.vbits = db->dev.vbits;
    P.k = db->info.k;
    P.n_values = db->info.n_values;
    P.tin = db->dev.tin;
    P.tout = db->dev.tout;
    P.sel_vi = sel_vi;
    P.with_desc = with_desc;
    return P;
}

struct gs_dbexport {
    int device = 0, k = 0;
    int32_t n_values = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    u64 *d_keys = nullptr;      // ascending
    uint32_t *d_vals = nullptr;
    // FASTQ text (gs_dbexport_fastq_*)
    uint8_t *d_names = nullptr, *d_project = nullptr, *d_text = nullptr;
    uint32_t *d_name_off = nullptr, *d_len = nullptr, *d_off = nullptr;
    void *d_scan = nullptr;
    size_t scan_bytes = 0, text_cap = 0;
    int64_t chunk_records = 0, next = -1;  // next record of the text (-1: gs_dbexport_fastq_begin first)
    int32_t project_len = 0;
};

static void dbexport_free_text(gs_dbexport *x) {
    for (void *p : {(void *)x->d_names, (void *)x->d_project, (void *)x->d_text, (void *)x->d_name_off, (void *)x->d_len, (void *)x->d_off, x->d_scan})
        gs_dev_free(p);
    x->d_names = x->d_project = x->d_text = nullptr;
    x->d_name_off = x->d_len = x->d_off = nullptr;
    x->d_scan = nullptr;
    x->next = -1;
}

static void dbexport_free(gs_dbexport *x) {
    hipSetDevice(x->device);
    if (x->stream) hipStreamSynchronize(x->stream);
    dbexport_free_text(x);
    gs_dev_free(x->d_keys);
    gs_dev_free(x->d_vals);
    if (x->stream) hipStreamDestroy(x->stream);
    delete x;
}

extern "C" int gs_db_value_counts(gs_db *db, int64_t *counts) {
    if (!db || !counts) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(db->device));
    const int32_t nv = db->info.n_values;
    hipStream_t stream = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    u64 *d = nullptr;
    hipError_t e = gs_dev_alloc((void **)&d, sizeof(u64) * ((size_t)nv + 1));
    GsExportParams P = export_params(db, -1, 0);
    P.count = d;
    P.hist = d + 1;
    if (e == hipSuccess) e = hipMemsetAsync(d, 0, sizeof(u64) * ((size_t)nv + 1), stream);
    if (e == hipSuccess) e = gs_launch_export_decode(&P, db->n_cu, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d + 1, sizeof(u64) * (size_t)nv, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    gs_dev_free(d);
    hipStreamDestroy(stream);
    if (e != hipSuccess) return hip_fail(e, "gs_db_value_counts");
    return GS_OK;
}

extern "C" int gs_dbexport_create(gs_dbexport **out, gs_db *db, int32_t sel_vi, int with_desc, int64_t *n_kmers) try {
    if (!out || !db) return fail(GS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (sel_vi < -1 || sel_vi >= db->info.n_values) return fail(GS_E_INVALID, "sel_vi out of range");
    HIP_TRY(hipSetDevice(db->device));
    gs_dbexport *x = new gs_dbexport();
    x->device = db->device;
    x->k = db->info.k;
    x->n_values = db->info.n_values;
    GsExportParams P = export_params(db, sel_vi, with_desc ? 1 : 0);
    u64 *d_count = nullptr, *keys_alt = nullptr;
    uint32_t *vals_alt = nullptr;
    u64 n = 0;
    auto step = [&](hipError_t e) { return e == hipSuccess; };
    hipError_t e = hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking);
    // pass 1 counts (the stripe's / partition's share is not in the info), pass 2 writes exactly that many
    if (step(e)) e = gs_dev_alloc((void **)&d_count, sizeof(u64));
    if (step(e)) e = hipMemsetAsync(d_count, 0, sizeof(u64), x->stream);
    P.count = d_count;
    if (step(e)) e = gs_launch_export_decode(&P, db->n_cu, x->stream);
    if (step(e)) e = hipMemcpyAsync(&n, d_count, sizeof(u64), hipMemcpyDeviceToHost, x->stream);
    if (step(e)) e = hipStreamSynchronize(x->stream);
    const size_t m = n ? (size_t)n : 1;
    if (step(e)) e = gs_dev_alloc((void **)&x->d_keys, m * sizeof(u64));
    if (step(e)) e = gs_dev_alloc((void **)&x->d_vals, m * sizeof(uint32_t));
    if (step(e)) e = gs_dev_alloc((void **)&keys_alt, m * sizeof(u64));
    if (step(e)) e = gs_dev_alloc((void **)&vals_alt, m * sizeof(uint32_t));
    if (step(e)) e = hipMemsetAsync(d_count, 0, sizeof(u64), x->stream);
    P.keys = x->d_keys;
    P.vals = x->d_vals;
    P.cap = n;
    u64 n2 = 0;
    if (step(e)) e = gs_launch_export_decode(&P, db->n_cu, x->stream);
    if (step(e)) e = hipMemcpyAsync(&n2, d_count, sizeof(u64), hipMemcpyDeviceToHost, x->stream);
    if (step(e)) e = hipStreamSynchronize(x->stream);
    u64 *ko = x->d_keys;
    uint32_t *vo = x->d_vals;
    if (step(e) && n2 == n) e = gs_build_sort(x->d_keys, keys_alt, x->d_vals, vals_alt, (int64_t)n, 2 * x->k, &ko, &vo, x->stream);
    gs_dev_free(d_count);
    if (e == hipSuccess) {  // keep the buffers the sorted pairs ended up in
        gs_dev_free(ko == x->d_keys ? keys_alt : x->d_keys);
        gs_dev_free(vo == x->d_vals ? vals_alt : x->d_vals);
        x->d_keys = ko;
        x->d_vals = vo;
    } else {
        gs_dev_free(keys_alt);
        gs_dev_free(vals_alt);
    }
    if (e != hipSuccess) {
        dbexport_free(x);
        return hip_fail(e, "gs_dbexport_create");
    }
    if (n2 != n) {
        dbexport_free(x);
        return fail(GS_E_HIP, "gs_dbexport_create: the two decode passes disagree");
    }
    x->n = (int64_t)n;
    if (n_kmers) *n_kmers = x->n;
    *out = x;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbexport_fetch(gs_dbexport *x, int64_t *kmers, int32_t *value_idx, int mem) {
    if (!x || (x->n > 0 && (!kmers || !value_idx))) return fail(GS_E_INVALID, "NULL argument");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HIP_TRY(hipSetDevice(x->device));
    if (x->n > 0) {
        const hipMemcpyKind kind = mem == GS_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        HIP_TRY(hipMemcpyAsync(kmers, x->d_keys, (size_t)x->n * sizeof(int64_t), kind, x->stream));
        HIP_TRY(hipMemcpyAsync(value_idx, x->d_vals, (size_t)x->n * sizeof(int32_t), kind, x->stream));
        HIP_TRY(hipStreamSynchronize(x->stream));
    }
    return GS_OK;
}

extern "C" int gs_dbexport_get_device(gs_dbexport *x, int *device) {
    if (!x || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = x->device;
    return GS_OK;
}

extern "C" int gs_dbexport_fastq_begin(gs_dbexport *x, const char *const *taxids, const char *project) try {
    if (!x || !taxids || !project) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(x->device));
    HIP_TRY(hipStreamSynchronize(x->stream));
    dbexport_free_text(x);
    std::vector<uint32_t> off((size_t)x->n_values + 1, 0);
    std::string names;
    size_t longest = 0;
    for (int32_t v = 0; v < x->n_values; v++) {
        const char *t = taxids[v] ? taxids[v] : "";
        const size_t l = strlen(t);
        names.append(t, l);
        longest = std::max(longest, l);
        if (names.size() >= ((size_t)1 << 32)) return fail(GS_E_INVALID, "taxid strings too long");
        off[(size_t)v + 1] = (uint32_t)names.size();
    }
    const size_t plen = strlen(project);
    if (plen > ((size_t)1 << 20) || longest > ((size_t)1 << 20)) return fail(GS_E_INVALID, "project name or taxid too long");
    // chunks of at most GS_EXPORT_CHUNK_BYTES of text (default 256 MiB), sized by the longest record
    size_t cap = (size_t)256 << 20;
    if (const char *e = getenv("GS_EXPORT_CHUNK_BYTES")) cap = (size_t)std::max(1LL, atoll(e));
    const size_t longest_rec = 20 + plen + longest + 20 + 2 * (size_t)x->k;
    cap = std::min(std::max(cap, longest_rec), (size_t)1 << 31);
    x->chunk_records = std::max<int64_t>(1, std::min<int64_t>((int64_t)(cap / longest_rec), std::max<int64_t>(x->n, 1)));
    x->text_cap = (size_t)x->chunk_records * longest_rec;
    x->project_len = (int32_t)plen;
    GsFastqParams P{};
    P.n = x->chunk_records;
    hipError_t e = gs_dev_alloc((void **)&x->d_names, names.size() + 1);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&x->d_name_off, off.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&x->d_project, plen + 1);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&x->d_len, ((size_t)x->chunk_records + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&x->d_off, ((size_t)x->chunk_records + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&x->d_text, x->text_cap);
    P.len = x->d_len;
    P.off = x->d_off;
    if (e == hipSuccess) e = gs_launch_export_fastq(&P, nullptr, &x->scan_bytes, nullptr, x->stream);
    if (e == hipSuccess) e = gs_dev_alloc(&x->d_scan, x->scan_bytes ? x->scan_bytes : 1);
    if (e == hipSuccess && !names.empty()) e = hipMemcpy(x->d_names, names.data(), names.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(x->d_name_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && plen) e = hipMemcpy(x->d_project, project, plen, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        dbexport_free_text(x);
        return hip_fail(e, "gs_dbexport_fastq_begin");
    }
    x->next = 0;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbexport_fastq_next(gs_dbexport *x, const uint8_t **d_text, int64_t *n_bytes, int64_t *n_records) {
    if (!x || !d_text || !n_bytes || !n_records) return fail(GS_E_INVALID, "NULL argument");
    if (x->next < 0) return fail(GS_E_STATE, "gs_dbexport_fastq_begin first");
    HIP_TRY(hipSetDevice(x->device));
    *d_text = x->d_text;
    *n_bytes = 0;
    *n_records = std::min<int64_t>(x->chunk_records, x->n - x->next);
    if (*n_records <= 0) {
        *n_records = 0;
        return GS_OK;
    }
    GsFastqParams P{};
    P.keys = x->d_keys;
    P.vals = x->d_vals;
    P.first = x->next;
    P.n = *n_records;
    P.k = x->k;
    P.project = x->d_project;
    P.project_len = x->project_len;
    P.names = x->d_names;
    P.name_off = x->d_name_off;
    P.len = x->d_len;
    P.off = x->d_off;
    int64_t bytes = 0;
    HIP_TRY(gs_launch_export_fastq(&P, x->d_scan, &x->scan_bytes, &bytes, x->stream));  // lengths + offsets
    if (bytes > (int64_t)x->text_cap) return fail(GS_E_HIP, "gs_dbexport_fastq_next: chunk larger than its buffer");
    P.text = x->d_text;
    HIP_TRY(gs_launch_export_fastq(&P, x->d_scan, &x->scan_bytes, &bytes, x->stream));  // the bytes
    *n_bytes = bytes;
    x->next += *n_records;
    return GS_OK;
}

extern "C" int gs_dbexport_destroy(gs_dbexport *x) {
    if (x) dbexport_free(x);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// match runs
// ---------------------------------------------------------------------------------------------------
// device state of the text mode (raw FASTQ chunk -> records, gs_text.hip); one per run / per filter handle
struct TextScan {
    // the chunk's bytes on the device: two buffers, filled by turns on a stream of their own, so that the copy of chunk
    // i+1 runs while the kernels of chunk i work on the other buffer.  d_text = the buffer of the latest chunk.
    uint8_t *d_text = nullptr;
    uint8_t *d_buf[2] = {nullptr, nullptr};
    size_t buf_cap[2] = {0, 0};
    hipStream_t copy_stream = nullptr;
    hipEvent_t done[2] = {};       // the kernels that read d_buf[b] have been issued up to here (on the owner's stream)
    bool done_valid[2] = {false, false};
    uint32_t *d_tile = nullptr, *d_nl = nullptr;
    size_t tile_cap = 0, nl_cap = 0;
    u64 *d_off2 = nullptr;
    size_t off2_cap = 0;
    // FASTA mode: per-line scan words, per-block totals, per-line destinations, the gathered sequences
    u64 *d_fa_scan = nullptr, *d_fa_block = nullptr;
    uint32_t *d_line_dst = nullptr;
    uint8_t *d_fa_seq = nullptr;
    size_t fa_scan_cap = 0, fa_block_cap = 0, line_dst_cap = 0, fa_seq_cap = 0;
    bool last_fasta = false;
    // general FASTQ (gs_match_submit_fastq_ml): per-line record structure
    uint32_t *d_ml_next = nullptr, *d_ml_plus = nullptr, *d_ml_ja = nullptr, *d_ml_jb = nullptr;
    uint8_t *d_ml_mark = nullptr, *d_ml_class = nullptr;
    u64 *d_ml_out = nullptr;
    size_t ml_next_cap = 0, ml_plus_cap = 0, ml_ja_cap = 0, ml_jb_cap = 0, ml_mark_cap = 0, ml_class_cap = 0;
    // GS_TEXT_BANKS independent streams of chunks (files read side by side): a refusal in one must not silence the
    // others, so the status words and totals exist once per bank; `bank` is the one the next calls work on
    uint32_t *d_status = nullptr;  // GS_TEXT_BANKS x GS_TS_WORDS
    u64 *d_totals = nullptr;       // GS_TEXT_BANKS x ([3] chunk scratch | [3] totals of the accepted chunks)
    int bank = 0;
    int64_t last_reads = 0, last_lines = 0;  // of the most recent chunk (per-read follow-up calls refer to it)
    hipEvent_t copied[8] = {};     // H2D of ticket t has completed: copied[t % 8]
    int64_t tickets = 0;
    // the writers' gather on the device (gs_*_compact_text, gs_deflate_dev.hip): output buffers [which][slot], per-record lengths,
    // per-block sums, page-locked totals; d_last_flags = where the last chunk's per-read flags lie on the device
    uint8_t *d_compact[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    size_t compact_cap[2][2] = {{0, 0}, {0, 0}};
    uint32_t *d_clen = nullptr;
    u64 *d_cblocks = nullptr, *h_ctotals = nullptr;
    size_t clen_cap = 0, cblocks_cap = 0;
    const uint8_t *d_last_flags = nullptr;
    const int32_t *d_last_class = nullptr;  // the same for its classes (gs_match_kraken_text)
    int64_t last_bytes = 0;
    bool last_four_line = false;
    bool last_ml = false;  // the last chunk was general FASTQ
    // the writers' text of FASTA and general FASTQ chunks (gs_*_compact_records, gs_rewrite.hip): the descriptor line of every record,
    // the quality lines gathered (scan words, per-block sums, destinations, bytes, bounds), offsets of the records' text, the text per
    // slot, totals and their page-locked landing area; the ticket of the chunk whose descriptor lines / qualities are in place
    uint32_t *d_rt_line = nullptr, *d_rt_piece = nullptr, *d_rt_qdst = nullptr;
    u64 *d_rt_out = nullptr, *d_rt_block = nullptr, *d_rt_qscan = nullptr, *d_rt_qblock = nullptr, *d_rt_qoff = nullptr;
    uint8_t *d_rt_qseq = nullptr;
    size_t rt_line_cap = 0, rt_piece_cap = 0, rt_qdst_cap = 0, rt_out_cap = 0, rt_block_cap = 0, rt_qscan_cap = 0, rt_qblock_cap = 0, rt_qoff_cap = 0,
           rt_qseq_cap = 0;
    u64 *d_rt_tot = nullptr, *h_rt_tot = nullptr;
    uint8_t *d_rt_text[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [which][slot], as d_compact
    size_t rt_text_cap[2][2] = {{0, 0}, {0, 0}};
    int64_t rt_heads_ticket = -1, rt_quals_ticket = -1;
};
enum { GS_TEXT_BANKS = 16 };

// `n` elements in place of what *p held (the caller has seen to it that nothing on the device uses the old block any more)
template <typename T>
static int renew(T **p, size_t n) {
    gs_dev_free(*p);
    *p = nullptr;
    HIP_TRY(gs_dev_alloc((void **)p, n * sizeof(T)));
    return GS_OK;
}

// room for `need` elements: a buffer that is too small goes once `stream` has drained, the new one holds `slack` elements more
template <typename T>
static int grow(T **p, size_t *cap, size_t need, hipStream_t stream, size_t slack) {
    if (*cap >= need) return GS_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    *cap = 0;
    const int rc = renew(p, need + slack);
    if (!rc) *cap = need + slack;
    return rc;
}
template <typename T>
static int grow(T **p, size_t *cap, size_t need, hipStream_t stream) {
    return grow(p, cap, need, stream, need / 4);
}

// device staging of a host batch (GS_MEM_HOST): the bases, the offsets and the per-read outputs.  One per filter handle, one per
// run for its synchronous calls (submit, submit_fixed, segments, text chunks with host outputs: they share it), one per async bank.
struct HostStage {
    const bool with_class;  // the matcher's; the filter keeps no d_class
    const bool slack;       // capacities: exactly the largest batch so far, or (the async banks, whose batches vary) a quarter on top
    explicit HostStage(bool with_class_ = true, bool slack_ = false) : with_class(with_class_), slack(slack_) {}
    uint8_t *d_seq = nullptr;
    uint64_t *d_off = nullptr;
    int32_t *d_class = nullptr;
    uint8_t *d_flags = nullptr;  // the filter: accept
    size_t seq_cap = 0, reads_cap = 0;  // reads_cap: entries of d_class / d_flags; d_off holds one more
    std::vector<uint64_t> rel;   // offsets of a batch whose offsets[0] != 0, rebased: the upload reads them after stage_upload has returned
};

// room for the offsets and per-read outputs of n_reads reads (a text chunk with host outputs needs no more).  Like stage_room it
// synchronises `stream` only when buffers have to go
static int stage_room_reads(HostStage &s, size_t n_reads, hipStream_t stream) {
    if (s.reads_cap >= n_reads) return GS_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    s.reads_cap = 0;
    const size_t cap = n_reads + (s.slack ? n_reads / 4 : 0);
    int rc = renew(&s.d_off, cap + 1);
    if (!rc && s.with_class) rc = renew(&s.d_class, cap);
    if (!rc) rc = renew(&s.d_flags, cap);
    if (!rc) s.reads_cap = cap;
    return rc;
}

// room for a batch of n_reads reads of nbytes bases; `also`: a second stream that uses the buffers, drained as well before one goes
static int stage_room(HostStage &s, size_t nbytes, size_t n_reads, hipStream_t stream, hipStream_t also = nullptr) {
    if (also && (s.seq_cap < nbytes + 1 || s.reads_cap < n_reads)) HIP_TRY(hipStreamSynchronize(also));
    const int rc = grow(&s.d_seq, &s.seq_cap, nbytes + 1, stream, s.slack ? nbytes / 4 : 0);
    return rc ? rc : stage_room_reads(s, n_reads, stream);
}

// the batch into d_seq / d_off on `stream`, the offsets rebased so that the staged slice starts at 0
static int stage_upload(HostStage &s, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, hipStream_t stream) {
    const uint64_t *hoff = offsets;
    if (offsets[0] != 0) {
        s.rel.resize((size_t)n_reads + 1);
        for (int64_t i = 0; i <= n_reads; i++) s.rel[(size_t)i] = offsets[i] - offsets[0];
        hoff = s.rel.data();
    }
    HIP_TRY(hipMemcpyAsync(s.d_seq, seq + offsets[0], (size_t)(offsets[n_reads] - offsets[0]), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s.d_off, hoff, sizeof(uint64_t) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, stream));
    return GS_OK;
}

// the per-read outputs the caller asked for, from the stage to its host arrays on `stream`
static int stage_download(const HostStage &s, int32_t *class_vi, uint8_t *flags, int64_t n_reads, hipStream_t stream) {
    if (class_vi) HIP_TRY(hipMemcpyAsync(class_vi, s.d_class, sizeof(int32_t) * (size_t)n_reads, hipMemcpyDeviceToHost, stream));
    if (flags) HIP_TRY(hipMemcpyAsync(flags, s.d_flags, (size_t)n_reads, hipMemcpyDeviceToHost, stream));
    return GS_OK;
}

static void stage_free(HostStage &s) {
    gs_dev_free(s.d_seq);
    gs_dev_free(s.d_off);
    gs_dev_free(s.d_class);
    gs_dev_free(s.d_flags);
}

// kernel time of a handle that profiles: an event pair around every timed launch, read out once the stream has passed it
struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;  // the pair of the launch under way
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    int64_t launches = 0;
    double total_ms = 0;
};

static int timer_start(KernelTimer &t, bool on, hipStream_t stream) {
    if (!on) return GS_OK;
    if (!t.e0) HIP_TRY(hipEventCreate(&t.e0));  // (left over: a launch that failed between start and stop)
    if (!t.e1) HIP_TRY(hipEventCreate(&t.e1));
    HIP_TRY(hipEventRecord(t.e0, stream));
    return GS_OK;
}

static int timer_stop(KernelTimer &t, bool on, hipStream_t stream) {
    if (!on) return GS_OK;
    HIP_TRY(hipEventRecord(t.e1, stream));
    t.pending.push_back({t.e0, t.e1});
    t.e0 = t.e1 = nullptr;
    return GS_OK;
}

// adds up the pairs handed in so far; the stream must have passed them
static int timer_collect(KernelTimer &t) {
    for (auto &p : t.pending) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.first, p.second));
        t.total_ms += ms;
        t.launches++;
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    t.pending.clear();
    return GS_OK;
}

static void timer_free(KernelTimer &t) {
    for (auto &p : t.pending) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    if (t.e0) hipEventDestroy(t.e0);
    if (t.e1) hipEventDestroy(t.e1);
    t = KernelTimer();
}

// gs_match_submit_async: two sets of device staging buffers, filled by turns on a copy stream, so that the copy of
// batch i+1 runs while the kernel of batch i works on the other set
struct BatchStage {
    HostStage bank[2] = {HostStage(true, true), HostStage(true, true)};
    hipStream_t copy_stream = nullptr;
    hipEvent_t copied[2] = {}, finished[4] = {};  // finished[t % 4]: everything of batch t is through
    int64_t tickets = 0;
};

struct gs_run {
    BatchStage stage;
    gs_db *db = nullptr;
    gs_match_cfg cfg{};
    hipStream_t stream = nullptr;
    int64_t *d_sums = nullptr;   // [stat_copies][n_values][GS_N_SUMS]; copy 0 is the one everything outside the kernels sees
    u64 *h_result = nullptr;     // page-locked landing area of gs_match_finish: sums | max keys | unique counts | double sums
    int64_t *d_max = nullptr;
    double *d_dsums = nullptr;
    u64 *d_route_cursors = nullptr;    // gs_match_encode_route: slots handed out per owner + overflow flag
    GsStatRec *d_stat_recs = nullptr;  // deferred statistics of the current batch (global-atomic counters only)
    u64 *d_stat_rec_count = nullptr;
    size_t stat_recs_cap = 0;
    int32_t *d_stat_vi = nullptr;      // the records' value indices as an array (stores with more values than one reduce pass takes)
    size_t stat_vi_cap = 0;
    bool use_stat_recs = false;
    // gates and quotients of a batch of one read length (GsQuotTable): built for (positions, both gate settings), uploaded once from
    // the page-locked copy and reused by every later batch of that length
    GsQuotTable *d_quot = nullptr, *h_quot = nullptr;
    hipEvent_t quot_copied = nullptr;  // the upload has left h_quot
    // the prefilter in front of the FIXED loop (gs_prefilter.hip): pf_mode is GS_PREFILTER (-1: the enabling rule decides); the
    // survivor count of a batch travels to a page-locked word (pf_h[slot], ~0 while the copy is under way) with the batch itself
    int pf_mode = -1;
    uint32_t *pf_h = nullptr;          // GS_PF_SLOTS words
    int64_t pf_slot_reads[4] = {0, 0, 0, 0};
    bool pf_slot_pending[4] = {false, false, false, false};
    int64_t pf_batches = 0;            // prefiltered batches so far (the next one takes slot pf_batches % 4)
    int pf_pause = 0;                  // batches that still go without the prefilter (the feedback rule)
    int64_t pf_last_survivors = -1, pf_last_reads = 0;  // of the last submitted batch; survivors -1: it went without the prefilter
    int pf_last_slot = -1;
    // the FIXED loop without the minimizer gate (gate_rule): gate_mode is GS_PF_GATE (-1: the rule decides; 1: every batch keeps the
    // gate; 0: every batch that can take that loop drops it); what the last submitted batch did, for gs_match_gate_info
    int gate_mode = -1;
    bool gate_last_gateless = false;
    double gate_last_pass = -1.0;
    // every read leaves the FIXED loop as a record (GsSnRec) or a row of node codes that gs_sn_reduce_kernel and gs_sn_walk_kernel
    // work off: sn_mode is GS_SN_DEFER (-1: not set, which is on; 0: such a batch takes the general loop); only runs whose
    // counters live in LDS (sn_lds) defer
    int sn_mode = -1;
    bool sn_lds = false;
    GsSnRec *d_sn_recs = nullptr;
    size_t sn_recs_cap = 0;
    uint16_t *d_sn_nodes = nullptr;    // [reads][GS_SN_ROW] node codes, sized as d_sn_recs
    size_t sn_nodes_cap = 0;
    uint32_t *d_sn_list = nullptr;     // the slots whose reads left as rows
    size_t sn_list_cap = 0;
    bool sn_last = false;              // the last submitted batch deferred (its count: word 7 of d_long_count)
    int quot_max = 0;                  // what the table was built for: positions (0: none yet) and the two gate settings
    double quot_tax = 0, quot_class = 0;
    int stat_copies = 1;         // > 1: global-atomic counters spread over several copies (GsMatchParams::stat_copies)
    bool stats_spread = false;   // some copy other than 0 may be non-zero: fold_stats() before reading
    uint32_t *d_hit_counts = nullptr;  // per slot, only when cfg.max_kmer_res_counts > 0
    uint32_t *d_bitmap = nullptr;  // compact copy of the slots' seen bits (built on demand: finish / device_state)
    int64_t bitmap_words = 0;
    bool seen_dirty = false;    // some slot may carry a seen bit
    bool bitmap_merged = false; // d_bitmap holds a merged (multi-rank) bitmap: do not re-extract
    bool bitmap_written = false; // d_bitmap of a store that is not striped may hold set bits (an extract, a merge)
    bool bitmap_stale = false;   // ... from before the last reset, which did not clear them (run_clear)
    u64 *d_result = nullptr;     // h_result's layout on the device: what gs_match_finish copies, in one piece
    u64 *d_unique = nullptr;     // (the unique counts inside d_result)
    unsigned int *d_long_count = nullptr;
    uint32_t *d_long_list = nullptr;
    int64_t long_cap = 0;
    int32_t *d_scratch = nullptr;  // long-read kernel: per wave tag[n_values] | cnt[n_values]
    uint32_t *d_serial = nullptr;
    // reads of tens of thousands of positions and more, taken apart over many waves (gs_match_huge_kernel): one allocation
    // [count u32 x 4 | list | heads | chunk records | cnt rows | first rows | touch rows]
    unsigned char *d_huge = nullptr;
    int huge_slots = 0, huge_min = GS_HUGE_MIN, huge_chunk_min = GS_HUGE_CHUNK_MIN;
    int long_grid = 0;
    HostStage host;  // host batches of the synchronous calls (GS_MEM_HOST)
    int grid = 0;
    // Kraken-style segments of the last gs_match_segments call
    uint32_t *d_seg_count = nullptr;
    u64 *d_seg_off = nullptr;
    int32_t *d_seg_code = nullptr, *d_seg_start = nullptr;
    int64_t seg_total = 0;
    TextScan text;  // text mode (gs_match_submit_text)
    KernelTimer timer;  // cfg.profile
    // Kraken-style lines as device text (gs_match_kraken_text): the taxid strings, the per-read arrays of the text kernels, the text
    // of the last call per slot, page-locked totals (bytes, lines)
    uint8_t *d_tax_bytes = nullptr;
    uint32_t *d_tax_off = nullptr;
    uint32_t *d_kr_name = nullptr;
    u64 *d_kr_rec = nullptr, *d_kr_blocks = nullptr, *d_kr_totals = nullptr, *h_kr_totals = nullptr;
    size_t kr_name_cap = 0, kr_rec_cap = 0, kr_blocks_cap = 0;
    uint8_t *d_kr_out[2] = {nullptr, nullptr};
    size_t kr_out_cap[2] = {0, 0};
    std::vector<uint64_t> kr_seg_off;
    KernelTimer kraken_timer;  // cfg.profile: the text kernels alone
};


static void text_free_fasta(TextScan &t) {
    gs_dev_free(t.d_ml_next);
    gs_dev_free(t.d_ml_plus);
    gs_dev_free(t.d_ml_ja);
    gs_dev_free(t.d_ml_jb);
    gs_dev_free(t.d_ml_mark);
    gs_dev_free(t.d_ml_class);
    gs_dev_free(t.d_ml_out);
    gs_dev_free(t.d_fa_scan);
    gs_dev_free(t.d_fa_block);
    gs_dev_free(t.d_line_dst);
    gs_dev_free(t.d_fa_seq);
}

static void text_free(TextScan &t) {
    text_free_fasta(t);
    if (t.copy_stream) {
        hipStreamSynchronize(t.copy_stream);
        hipStreamDestroy(t.copy_stream);
    }
    for (hipEvent_t ev : t.done)
        if (ev) hipEventDestroy(ev);
    gs_dev_free(t.d_buf[0]);
    gs_dev_free(t.d_buf[1]);
    gs_dev_free(t.d_tile);
    gs_dev_free(t.d_nl);
    gs_dev_free(t.d_off2);
    gs_dev_free(t.d_status);
    gs_dev_free(t.d_totals);
    for (auto &w : t.d_compact)
        for (uint8_t *q : w) gs_dev_free(q);
    gs_dev_free(t.d_clen);
    gs_dev_free(t.d_cblocks);
    if (t.h_ctotals) hipHostFree(t.h_ctotals);
    gs_dev_free(t.d_rt_line);
    gs_dev_free(t.d_rt_piece);
    gs_dev_free(t.d_rt_qdst);
    gs_dev_free(t.d_rt_out);
    gs_dev_free(t.d_rt_block);
    gs_dev_free(t.d_rt_qscan);
    gs_dev_free(t.d_rt_qblock);
    gs_dev_free(t.d_rt_qoff);
    gs_dev_free(t.d_rt_qseq);
    gs_dev_free(t.d_rt_tot);
    if (t.h_rt_tot) hipHostFree(t.h_rt_tot);
    for (auto &w : t.d_rt_text)
        for (uint8_t *q : w) gs_dev_free(q);
    for (hipEvent_t ev : t.copied)
        if (ev) hipEventDestroy(ev);
    t = TextScan();
}

static int text_reset_bank(TextScan &t, int bank, bool totals, hipStream_t stream) {
    uint32_t *st = t.d_status + (size_t)bank * GS_TS_WORDS;
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(uint32_t) * GS_TS_WORDS, stream));
    HIP_TRY(hipMemsetAsync(st + GS_TS_FIRST_BAD, 0xff, sizeof(uint32_t), stream));
    if (totals) HIP_TRY(hipMemsetAsync(t.d_totals + (size_t)bank * 6, 0, sizeof(u64) * 6, stream));
    return GS_OK;
}

// the selected bank, or (all = true: begin / reset of the handle) every bank
static int text_reset(TextScan &t, bool totals, hipStream_t stream, bool all = false) {
    if (!t.d_status) return GS_OK;
    if (!all) return text_reset_bank(t, t.bank, totals, stream);
    for (int b = 0; b < GS_TEXT_BANKS; b++) {
        int rc = text_reset_bank(t, b, totals, stream);
        if (rc) return rc;
    }
    return GS_OK;
}

// copies the chunk to the device and runs the record scan; *ticket identifies the chunk.  After it the (start, end)
// pairs of the sequence lines are in t.d_off2, the newline offsets in t.d_nl and the skip flag in t.d_status.
// fasta_records < 0: four-line FASTQ; >= 0: FASTA with that many header lines (gs_text.hip)
// ml_out != nullptr: general FASTQ -- the record structure is found on the device first (this call then waits for it) and
// ml_out[0] = complete records (-1: the chunk was refused), ml_out[1] = bytes, ml_out[2] = lines they cover
// goal != nullptr (fasta2fastq, with fasta_records): only the newlines are found here, the lines are read under the goal's own
// rule (gs_rewrite.hip, goal mode) -- the shared fields of *goal are filled in -- and the chunk is committed
static int text_submit(TextScan &t, hipStream_t stream, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int k,
                       int64_t *ticket, int64_t fasta_records = -1, int64_t *ml_out = nullptr, GsRewriteParams *goal = nullptr) {
    const bool ml = ml_out != nullptr;
    const bool fasta = fasta_records >= 0 || ml;
    if (ml) {
        ml_out[0] = ml_out[1] = ml_out[2] = 0;
        fasta_records = 0;
    }
    if (n_bytes < 0 || n_lines < 0 || (!fasta && (n_lines & 3) != 0) || (n_bytes > 0 && !text) || n_lines > n_bytes)
        return fail(GS_E_INVALID, "bad text chunk (n_lines must be a multiple of 4)");
    if (ml && n_lines >= ((int64_t)1 << 26)) return fail(GS_E_INVALID, "general FASTQ chunks are limited to 2^26 lines");
    if (fasta && (fasta_records > n_lines || fasta_records >= ((int64_t)1 << 24)))
        return fail(GS_E_INVALID, "bad FASTA chunk (at most 2^24 - 1 records, not more records than lines)");
    if (n_bytes > ((int64_t)1 << 30)) return fail(GS_E_INVALID, "text chunks are limited to 1 GiB");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (!t.d_status) {
        HIP_TRY(gs_dev_alloc((void **)&t.d_status, sizeof(uint32_t) * GS_TS_WORDS * GS_TEXT_BANKS));
        HIP_TRY(gs_dev_alloc((void **)&t.d_totals, sizeof(u64) * 6 * GS_TEXT_BANKS));
        int rc = text_reset(t, true, stream, true);
        if (rc) return rc;
        for (hipEvent_t &ev : t.copied) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (hipEvent_t &ev : t.done) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipStreamCreateWithFlags(&t.copy_stream, hipStreamNonBlocking));
    }
    int64_t n_reads = ml ? n_lines / 4 + 1 : (fasta ? fasta_records : (n_lines >> 2));  // (ml: an upper bound for now)
    const size_t padded = ((size_t)n_bytes + 4095) & ~(size_t)4095;
    const int64_t tk = t.tickets;
    const int b = (int)(tk & 1);
    int rc;
    if (t.buf_cap[b] < padded + 4096) HIP_TRY(hipStreamSynchronize(t.copy_stream));  // (grow() waits for `stream` itself)
    if ((rc = grow(&t.d_buf[b], &t.buf_cap[b], padded + 4096, stream))) return rc;
    if ((rc = grow(&t.d_tile, &t.tile_cap, padded / 4096 + 1, stream))) return rc;
    if ((rc = grow(&t.d_nl, &t.nl_cap, (size_t)n_lines + 4, stream))) return rc;
    if ((rc = grow(&t.d_off2, &t.off2_cap, 2 * (size_t)n_reads + 2, stream))) return rc;
    if (fasta) {
        if ((rc = grow(&t.d_fa_scan, &t.fa_scan_cap, (size_t)n_lines + 1, stream))) return rc;
        if ((rc = grow(&t.d_fa_block, &t.fa_block_cap, (size_t)n_lines / GS_FA_BLOCK + 2, stream))) return rc;
        if ((rc = grow(&t.d_line_dst, &t.line_dst_cap, (size_t)n_lines + 1, stream))) return rc;
        if ((rc = grow(&t.d_fa_seq, &t.fa_seq_cap, (size_t)n_bytes + 256, stream))) return rc;
    }
    if (ml) {
        const size_t nl1 = (size_t)n_lines + 1;
        if ((rc = grow(&t.d_ml_next, &t.ml_next_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_ml_plus, &t.ml_plus_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_ml_ja, &t.ml_ja_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_ml_jb, &t.ml_jb_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_ml_mark, &t.ml_mark_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_ml_class, &t.ml_class_cap, nl1, stream))) return rc;
        if (!t.d_ml_out) HIP_TRY(gs_dev_alloc((void **)&t.d_ml_out, sizeof(u64) * 4));
    }
    t.d_text = t.d_buf[b];
    // the copy waits for the kernels of the chunk before last (they read this buffer), the scan for the copy
    if (t.done_valid[b]) HIP_TRY(hipStreamWaitEvent(t.copy_stream, t.done[b], 0));
    if (n_bytes > 0)
        HIP_TRY(hipMemcpyAsync(t.d_text, text, (size_t)n_bytes, mem == GS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                               t.copy_stream));
    HIP_TRY(hipEventRecord(t.copied[tk & 7], t.copy_stream));
    HIP_TRY(hipStreamWaitEvent(stream, t.copied[tk & 7], 0));
    if (padded > (size_t)n_bytes) HIP_TRY(hipMemsetAsync(t.d_text + n_bytes, ' ', padded - (size_t)n_bytes, stream));
    GsTextParams T{};
    T.text = t.d_text;
    T.n_bytes = n_bytes;
    T.n_lines = n_lines;
    T.tile_count = t.d_tile;
    T.nl = t.d_nl;
    T.off2 = (unsigned long long *)t.d_off2;
    T.chunk_totals = (unsigned long long *)t.d_totals + (size_t)t.bank * 6;
    T.run_totals = T.chunk_totals + 3;
    T.status = t.d_status + (size_t)t.bank * GS_TS_WORDS;
    T.k = k;
    T.n_records = fasta ? fasta_records : -1;
    T.fa_scan = (unsigned long long *)t.d_fa_scan;
    T.fa_block = (unsigned long long *)t.d_fa_block;
    T.line_dst = t.d_line_dst;
    T.fa_seq = t.d_fa_seq;
    t.last_fasta = fasta;
    if (ml) {
        // first half: newlines + record structure; then this thread waits for the counts (the match launch needs the number
        // of reads, the caller the bytes that belong to the next chunk)
        T.ml_next = t.d_ml_next;
        T.ml_plus = t.d_ml_plus;
        T.ml_jump_a = t.d_ml_ja;
        T.ml_jump_b = t.d_ml_jb;
        T.ml_mark = t.d_ml_mark;
        T.ml_out = (unsigned long long *)t.d_ml_out;
        const u64 init[4] = {0, (u64)n_lines, 0, 0};
        HIP_TRY(hipMemcpyAsync(t.d_ml_out, init, sizeof(init), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(t.d_ml_class, 0, (size_t)n_lines + 1, stream));
        HIP_TRY(gs_launch_text_ml(&T, t.d_ml_class, stream));
        u64 got[4] = {0, 0, 0, 0};
        uint32_t st[GS_TS_WORDS];
        HIP_TRY(hipMemcpyAsync(got, t.d_ml_out, sizeof(got), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(st, T.status, sizeof(st), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        int64_t lines_done = 0, bytes_done = 0;
        n_reads = 0;
        if (st[GS_TS_CHUNK_ERR] == 0 && st[GS_TS_STICKY] == 0 && n_lines > 0) {
            n_reads = (int64_t)got[0];
            lines_done = (int64_t)got[1];
            if (lines_done > 0) {
                uint32_t last_nl = 0;
                HIP_TRY(hipMemcpy(&last_nl, t.d_nl + (lines_done - 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
                bytes_done = (int64_t)last_nl + 1;
            }
        }
        ml_out[0] = (st[GS_TS_CHUNK_ERR] != 0 || st[GS_TS_STICKY] != 0) ? -1 : n_reads;
        ml_out[1] = bytes_done;
        ml_out[2] = lines_done;
        // second half on what is whole: the FASTA kernels under the line classes (or, after an error, only the commit)
        T.n_lines = lines_done;
        T.n_bytes = bytes_done > 0 ? bytes_done : n_bytes;
        T.n_records = n_reads;
        T.line_class = t.d_ml_class;
        n_lines = lines_done;
    }
    if (goal) {
        goal->text = T.text;
        goal->nl = T.nl;
        goal->fa_scan = T.fa_scan;
        goal->fa_block = T.fa_block;
        goal->line_dst = T.line_dst;
        goal->fa_seq = T.fa_seq;
        goal->off2 = T.off2;
        goal->status = T.status;
        goal->gate = T.status + GS_TS_CHUNK_ERR;
        HIP_TRY(gs_launch_text_lines(&T, stream));
        HIP_TRY(gs_launch_rewrite_lines(goal, stream));
        HIP_TRY(gs_launch_text_commit(&T, (uint32_t)tk, stream));
        goal->gate = T.status + GS_TS_SKIP;
    } else {
        HIP_TRY(gs_launch_text_scan(&T, (uint32_t)tk, stream));
    }
    HIP_TRY(hipEventRecord(t.done[b], stream));
    t.done_valid[b] = true;
    t.tickets = tk + 1;
    t.last_reads = n_reads;
    t.last_lines = n_lines;
    t.last_bytes = n_bytes;
    t.last_four_line = !fasta;
    t.last_ml = ml;
    t.d_last_flags = nullptr;
    t.d_last_class = nullptr;
    if (ticket) *ticket = tk;
    return GS_OK;
}

static int text_touched(TextScan &t, hipStream_t stream);

// the records of the last chunk whose flag says so, as ReadEntry.write writes them, into t.d_compact[which][slot]; synchronises
static int text_compact(TextScan &t, hipStream_t stream, int mask, int want, int which, int slot, int with_probs, const uint8_t **d_out, int64_t *n_bytes,
                        int64_t *n_records) {
    if (!d_out || !n_bytes || !n_records) return fail(GS_E_INVALID, "NULL argument");
    *d_out = nullptr;
    *n_bytes = *n_records = 0;
    if (which < 0 || which > 1 || slot < 0 || slot > 1) return fail(GS_E_INVALID, "which and slot must be 0 or 1");
    if (t.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    if (!t.last_four_line) return fail(GS_E_STATE, "the last chunk was not four-line FASTQ");
    if (!t.d_last_flags) return fail(GS_E_STATE, "the last chunk was submitted without per-read flags");
    const int64_t n = t.last_reads;
    if (n == 0) return GS_OK;
    int rc;
    if ((rc = grow(&t.d_compact[which][slot], &t.compact_cap[which][slot], (size_t)t.last_bytes + 64, stream))) return rc;
    if ((rc = grow(&t.d_clen, &t.clen_cap, (size_t)n, stream))) return rc;
    if ((rc = grow(&t.d_cblocks, &t.cblocks_cap, 2 * ((size_t)n / 256 + 1) + 2, stream))) return rc;
    if (!t.h_ctotals) HIP_TRY(hipHostMalloc((void **)&t.h_ctotals, 2 * sizeof(u64)));
    if (gs_compact_records_device(stream, t.d_text, t.d_nl, n, t.d_last_flags, mask, want, with_probs, t.d_compact[which][slot], t.d_clen, t.d_cblocks, t.h_ctotals) != GS_OK)
        return fail(GS_E_HIP, std::string("record gather: ") + gs_deflate_last_error());
    if ((rc = text_touched(t, stream))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    *d_out = t.d_compact[which][slot];
    *n_bytes = (int64_t)t.h_ctotals[0];
    *n_records = (int64_t)t.h_ctotals[1];
    return GS_OK;
}

// to be called after every launch on `stream` that reads the latest chunk's bytes (match / filter / segment kernels):
// the buffer may be overwritten by the chunk after next only when these are through
static int text_touched(TextScan &t, hipStream_t stream) {
    if (t.tickets == 0) return GS_OK;
    HIP_TRY(hipEventRecord(t.done[(t.tickets - 1) & 1], stream));
    return GS_OK;
}

// what a text chunk hands to the kernel of its handle (match or filter)
struct TextBatch {
    int64_t n_reads = 0;
    bool fasta = false;               // the reads were gathered (FASTA, general FASTQ), not left in place
    const uint8_t *d_seq = nullptr;   // FASTQ: the sequence lines in place, (start, end) pairs; FASTA: the gathered sequences, running offsets
    int off_stride = 2;
    const uint32_t *d_skip = nullptr; // the bank's skip flag: a refused chunk is not worked on
    bool dev_out = false;             // the per-read outputs are device arrays (GS_MEM_DEVICE_TEXT: the text is in HBM, they are host arrays)
};

// front half of a text-mode submit: checks mem, copies and scans the chunk (text_submit) and says what to launch on; n_reads == 0: nothing
static int text_batch(TextScan &t, hipStream_t stream, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int k, int64_t *ticket,
                      int64_t fasta_records, int64_t *ml_out, TextBatch *tb) {
    tb->fasta = fasta_records >= 0 || ml_out != nullptr;
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE && mem != GS_MEM_DEVICE_TEXT) return fail(GS_E_INVALID, "bad mem");
    const int rc = text_submit(t, stream, text, n_bytes, n_lines, mem == GS_MEM_HOST ? GS_MEM_HOST : GS_MEM_DEVICE, k, ticket, fasta_records, ml_out);
    if (rc) return rc;
    tb->n_reads = ml_out ? std::max<int64_t>(ml_out[0], 0) : (tb->fasta ? fasta_records : (n_lines >> 2));
    tb->dev_out = mem == GS_MEM_DEVICE;
    tb->d_seq = tb->fasta ? t.d_fa_seq : t.d_text;
    tb->off_stride = tb->fasta ? 1 : 2;
    tb->d_skip = t.d_status + (size_t)t.bank * GS_TS_WORDS + GS_TS_SKIP;
    return GS_OK;
}

// the text of a chunk's records is at most twice the chunk and five bytes per record (descriptor and read stand in the chunk, the
// tail is as long as the read or stands in the chunk as well); a multiple of 16 with room behind the text
static size_t reads_bound(int64_t n_bytes, int64_t n_records) { return ((2 * (size_t)n_bytes + 5 * (size_t)n_records + 15) & ~(size_t)15) + 64; }

// GS_OK when the last chunk is one whose records lie gathered (FASTA, general FASTQ) and was not refused; synchronises
static int records_state(TextScan &t, hipStream_t stream) {
    if (t.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    if (t.last_four_line) return fail(GS_E_STATE, "the last chunk was four-line FASTQ");
    uint32_t skip = 0;
    HIP_TRY(hipMemcpyAsync(&skip, t.d_status + (size_t)t.bank * GS_TS_WORDS + GS_TS_SKIP, sizeof(skip), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (skip) return fail(GS_E_STATE, "the last chunk was refused");
    return GS_OK;
}

// what the rewrite kernels take from the latest chunk, a FASTA or general FASTQ one (ReadEntry mode)
static void records_params(TextScan &t, GsRewriteParams *R) {
    R->text = t.d_text;
    R->n_lines = t.last_lines;  // (general FASTQ: the lines of its whole records)
    R->n_records = t.last_reads;
    R->nl = t.d_nl;
    R->line_class = t.last_ml ? t.d_ml_class : nullptr;
    R->fa_scan = (unsigned long long *)t.d_fa_scan;
    R->fa_block = (unsigned long long *)t.d_fa_block;
    R->line_dst = t.d_line_dst;
    R->fa_seq = t.d_fa_seq;
    R->off2 = (unsigned long long *)t.d_off2;
    R->status = t.d_status + (size_t)t.bank * GS_TS_WORDS;
    R->gate = R->status + GS_TS_SKIP;
    R->keep_first = t.last_ml ? 1 : 0;
    R->rec_line = t.d_rt_line;
    R->rec_out = (unsigned long long *)t.d_rt_out;
    R->rec_block = (unsigned long long *)t.d_rt_block;
    R->piece_rec = t.d_rt_piece;
    R->totals = (unsigned long long *)t.d_rt_tot;
}

// the descriptor line of every record of the latest chunk in t.d_rt_line (once per chunk)
static int records_heads(TextScan &t, hipStream_t stream) {
    if (t.rt_heads_ticket == t.tickets) return GS_OK;
    int rc = grow(&t.d_rt_line, &t.rt_line_cap, (size_t)t.last_reads + 1, stream);
    if (rc) return rc;
    GsRewriteParams R{};
    records_params(t, &R);
    HIP_TRY(gs_launch_rewrite_heads(&R, stream));
    t.rt_heads_ticket = t.tickets;
    return GS_OK;
}

// the records of the last chunk, a FASTA or general FASTQ one, whose flag says so -- ((flags[r] & mask) != 0) == (want != 0) -- as
// ReadEntry.write writes them, into t.d_rt_text[which][slot] (which: the filter's two files, which are written side by side);
// synchronises.  timer (may be nullptr): the launches run between its events
static int text_records(TextScan &t, hipStream_t stream, int n_cu, int mask, int want, int which, int with_probs, int slot, KernelTimer *timer, bool profile,
                        const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) {
    if (!d_out || !n_bytes || !n_records) return fail(GS_E_INVALID, "NULL argument");
    *d_out = nullptr;
    *n_bytes = *n_records = 0;
    if (slot < 0 || slot > 1) return fail(GS_E_INVALID, "slot must be 0 or 1");
    int rc = records_state(t, stream);
    if (rc) return rc;
    const int64_t n = t.last_reads;
    if (n == 0) return GS_OK;
    if (!t.d_last_flags) return fail(GS_E_STATE, "the last chunk was submitted without per-read flags");
    const bool quals = with_probs != 0 && t.last_ml;  // (a FASTA record has no qualities: '~' either way)
    const size_t bound = reads_bound(t.last_bytes, n);
    if ((rc = grow(&t.d_rt_line, &t.rt_line_cap, (size_t)n + 1, stream))) return rc;
    if ((rc = grow(&t.d_rt_out, &t.rt_out_cap, (size_t)n + 1, stream))) return rc;
    if ((rc = grow(&t.d_rt_block, &t.rt_block_cap, (size_t)n / 256 + 2, stream))) return rc;
    if ((rc = grow(&t.d_rt_piece, &t.rt_piece_cap, bound / 4096 + 2, stream))) return rc;
    if ((rc = grow(&t.d_rt_text[which][slot], &t.rt_text_cap[which][slot], bound, stream))) return rc;
    if (!t.d_rt_tot) HIP_TRY(gs_dev_alloc((void **)&t.d_rt_tot, sizeof(u64) * 4));
    if (!t.h_rt_tot) HIP_TRY(hipHostMalloc((void **)&t.h_rt_tot, sizeof(u64) * 4));
    const bool gather = quals && t.rt_quals_ticket != t.tickets;
    if (gather) {
        const size_t nl1 = (size_t)t.last_lines + 1;
        if ((rc = grow(&t.d_rt_qscan, &t.rt_qscan_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_rt_qblock, &t.rt_qblock_cap, nl1 / 256 + 2, stream))) return rc;
        if ((rc = grow(&t.d_rt_qdst, &t.rt_qdst_cap, nl1, stream))) return rc;
        if ((rc = grow(&t.d_rt_qseq, &t.rt_qseq_cap, (size_t)t.last_bytes + 256, stream))) return rc;
        if ((rc = grow(&t.d_rt_qoff, &t.rt_qoff_cap, (size_t)n + 1, stream))) return rc;
    }
    HIP_TRY(hipMemsetAsync(t.d_rt_tot, 0, sizeof(u64) * 4, stream));
    GsRewriteParams R{};
    records_params(t, &R);
    if (timer && (rc = timer_start(*timer, profile, stream))) return rc;
    if (gather) {  // the quality lines; the pass finds the descriptor lines too
        GsRewriteParams Q = R;
        Q.goal_mode = 2;
        Q.fa_scan = (unsigned long long *)t.d_rt_qscan;
        Q.fa_block = (unsigned long long *)t.d_rt_qblock;
        Q.line_dst = t.d_rt_qdst;
        Q.fa_seq = t.d_rt_qseq;
        Q.off2 = (unsigned long long *)t.d_rt_qoff;
        HIP_TRY(gs_launch_rewrite_lines(&Q, stream));
        t.rt_quals_ticket = t.rt_heads_ticket = t.tickets;
    } else if ((rc = records_heads(t, stream)))
        return rc;
    if (quals) {
        R.q_seq = t.d_rt_qseq;
        R.q_off = (const unsigned long long *)t.d_rt_qoff;
    }
    R.flags = t.d_last_flags;
    R.flag_mask = (uint32_t)mask;
    R.flag_want = want != 0;
    R.out = t.d_rt_text[which][slot];
    HIP_TRY(gs_launch_rewrite_copy(&R, (int64_t)bound - 64, n_cu, stream));
    if (timer && (rc = timer_stop(*timer, profile, stream))) return rc;
    if ((rc = text_touched(t, stream))) return rc;
    HIP_TRY(hipMemcpyAsync(t.h_rt_tot, t.d_rt_tot, sizeof(u64) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n_bytes = (int64_t)t.h_rt_tot[0];
    *n_records = (int64_t)t.h_rt_tot[1];
    *d_out = *n_bytes > 0 ? t.d_rt_text[which][slot] : nullptr;
    return GS_OK;
}

// what a general FASTQ chunk reports: complete records, the bytes and the lines they cover (text_submit's ml_out)
static int ml_report(int rc, const int64_t out[3], int64_t *n_records, int64_t *consumed_bytes, int64_t *consumed_lines) {
    *n_records = out[0];
    *consumed_bytes = out[1];
    if (consumed_lines) *consumed_lines = out[2];
    return rc;
}

static int text_wait_copy(TextScan &t, int64_t ticket) {
    if (ticket < 0 || ticket >= t.tickets) return fail(GS_E_INVALID, "unknown ticket");
    if (ticket + 8 <= t.tickets) return GS_OK;  // its event has been re-recorded by a later submit: long done
    HIP_TRY(hipEventSynchronize(t.copied[ticket & 7]));
    return GS_OK;
}

// synchronises the stream
static int text_status(TextScan &t, hipStream_t stream, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]) {
    if (failed_ticket) *failed_ticket = -1;
    if (first_bad_record) *first_bad_record = -1;
    if (totals) totals[0] = totals[1] = totals[2] = 0;
    if (!t.d_status) return GS_OK;
    uint32_t st[GS_TS_WORDS];
    u64 tt[6];
    HIP_TRY(hipMemcpyAsync(st, t.d_status + (size_t)t.bank * GS_TS_WORDS, sizeof(st), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(tt, t.d_totals + (size_t)t.bank * 6, sizeof(tt), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (st[GS_TS_STICKY]) {
        if (failed_ticket) *failed_ticket = (int64_t)st[GS_TS_FAILED_TICKET];
        if (first_bad_record && st[GS_TS_FIRST_BAD] != 0xffffffffu) *first_bad_record = (int64_t)st[GS_TS_FIRST_BAD];
    }
    if (totals)
        for (int i = 0; i < 3; i++) totals[i] = (int64_t)tt[3 + i];
    return GS_OK;
}

// (start, end) of the reads of the most recent chunk, a FASTA one (`four_line`: the caller's words for the other kind); synchronises
static int text_read_bounds(TextScan &t, hipStream_t stream, uint64_t *bounds, const char *four_line) {
    if (t.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    if (!t.last_fasta) return fail(GS_E_STATE, four_line);
    HIP_TRY(hipMemcpyAsync(bounds, t.d_off2, sizeof(uint64_t) * ((size_t)t.last_reads + 1), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GS_OK;
}

// the line classes of the most recent general FASTQ chunk; synchronises
static int text_line_classes(TextScan &t, hipStream_t stream, uint8_t *classes) {
    if (t.tickets == 0 || !t.d_ml_class) return fail(GS_E_STATE, "no general FASTQ chunk has been submitted");
    if (t.last_lines > 0) HIP_TRY(hipMemcpyAsync(classes, t.d_ml_class, (size_t)t.last_lines, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GS_OK;
}

static int run_clear(gs_run *run) {
    const size_t nv = (size_t)run->db->info.n_values;
    const size_t cp = (size_t)run->stat_copies;
    // (sums, max keys, double sums and the long-read queue counters [queue length, consumer cursor] are one block)
    HIP_TRY(hipMemsetAsync(run->d_sums, 0, sizeof(int64_t) * nv * (GS_N_SUMS + 1 + GS_N_DCOLS) * cp + 2 * sizeof(unsigned int), run->stream));
    run->stats_spread = false;
    // The compact bitmap of a store that is not striped is a COPY of the seen bits in the store: whoever reads it (gs_match_finish,
    // gs_match_device_state, gs_match_merge) first has an extract sweep write every one of its words, unless bitmap_merged says
    // that it holds a merge -- and bitmap_merged is cleared below.  So the bits of an earlier round are never read and need no
    // clearing here (one word per 32 slots and per record bucket: 512 MiB on a 473 M-k-mer store).  The one reader that does
    // not extract, gs_match_or_bitmap, clears a stale bitmap itself (bitmap_settle).  The kernels of a striped store write
    // their seen bits into the bitmap: there it is the state itself and is cleared.
    if (run->db->striped())
        HIP_TRY(hipMemsetAsync(run->d_bitmap, 0, sizeof(uint32_t) * (size_t)run->bitmap_words, run->stream));
    else
        run->bitmap_stale = run->bitmap_written;
    if (run->d_hit_counts)
        HIP_TRY(hipMemsetAsync(run->d_hit_counts, 0, sizeof(uint32_t) * (size_t)(run->db->n_slots() + run->db->n_rec * GS_REC_SLOTS), run->stream));
    if (run->seen_dirty && !run->db->striped())  // (a striped store's seen bits are the bitmap that was just cleared)
        HIP_TRY(gs_launch_clear_seen(run->db->d_table, run->db->n_slots(), run->db->d_rec, run->db->n_rec, run->stream));
    run->seen_dirty = false;
    run->bitmap_merged = false;
    return GS_OK;
}

static void run_free(gs_run *run) {
    if (!run) return;
    hipSetDevice(run->db->device);
    timer_free(run->timer);
    hipHostFree(run->h_result);
    gs_dev_free(run->d_sums);  // (d_max, d_dsums, d_long_count lie inside)
    gs_dev_free(run->d_stat_recs);
    gs_dev_free(run->d_stat_vi);
    gs_dev_free(run->d_stat_rec_count);
    gs_dev_free(run->d_sn_recs);
    gs_dev_free(run->d_sn_nodes);
    gs_dev_free(run->d_sn_list);
    gs_dev_free(run->d_quot);
    hipHostFree(run->h_quot);
    hipHostFree(run->pf_h);
    if (run->quot_copied) hipEventDestroy(run->quot_copied);
    gs_dev_free(run->d_route_cursors);
    gs_dev_free(run->d_bitmap);
    gs_dev_free(run->d_hit_counts);
    gs_dev_free(run->d_result);  // (d_unique lies inside)
    gs_dev_free(run->d_long_list);
    gs_dev_free(run->d_scratch);
    gs_dev_free(run->d_serial);
    gs_dev_free(run->d_huge);
    stage_free(run->host);
    gs_dev_free(run->d_seg_count);
    gs_dev_free(run->d_seg_off);
    gs_dev_free(run->d_seg_code);
    gs_dev_free(run->d_seg_start);
    timer_free(run->kraken_timer);
    gs_dev_free(run->d_tax_bytes);
    gs_dev_free(run->d_tax_off);
    gs_dev_free(run->d_kr_name);
    gs_dev_free(run->d_kr_rec);
    gs_dev_free(run->d_kr_blocks);
    gs_dev_free(run->d_kr_totals);
    hipHostFree(run->h_kr_totals);
    gs_dev_free(run->d_kr_out[0]);
    gs_dev_free(run->d_kr_out[1]);
    text_free(run->text);
    {
        BatchStage &g = run->stage;
        if (g.copy_stream) {
            hipStreamSynchronize(g.copy_stream);
            hipStreamDestroy(g.copy_stream);
        }
        for (int b = 0; b < 2; b++) {
            stage_free(g.bank[b]);
            if (g.copied[b]) hipEventDestroy(g.copied[b]);
        }
        for (hipEvent_t ev : g.finished)
            if (ev) hipEventDestroy(ev);
    }
    if (run->stream) hipStreamDestroy(run->stream);
    delete run;
}

// ---- the sampled 15-mer prefilter (gs_prefilter.h) -- THE ENABLING RULE, all of it:
// a store gets a filter, and a batch of m samples per read goes through it, only if a read of uniform random bases is predicted to
// pass with a probability below GS_PF_MAX_PASS: 1 - (1 - |S| / 2^29)^m (2^29 canonical 15-mers exist).  GS_PREFILTER=0 / 1 overrides
// the rule (read per run: tests and A/B runs take both paths from one library).  Striped and partitioned stores and stores without
// records get no filter.  The feedback rule for streams that are mostly hits is next to it: a batch of which more than
// GS_PF_HIT_RICH of the reads survived sends the next GS_PF_PAUSE batches straight to the match kernel.
#define GS_PF_MAX_PASS 0.5
#define GS_PF_HIT_RICH 0.85
#define GS_PF_PAUSE 15
#define GS_PF_SLOTS 4
// the predicted pass probability of a read of uniform random bases; a store whose 15-mers were never counted passes everything
static double prefilter_pass(int64_t n_lmers, int samples) {
    if (n_lmers < 0) return 1.0;
    return 1.0 - std::pow(1.0 - (double)n_lmers / (double)(1LL << 29), (double)samples);
}
static bool prefilter_rule(const gs_db *db, int mode, int samples) {
    if (mode == 0 || !db->d_pf || db->pf_set < 0) return false;
    if (mode > 0) return true;
    return prefilter_pass(db->pf_set, samples) < GS_PF_MAX_PASS;
}
// ---- THE GATE RULE, all of it: a batch that goes through the prefilter (or that the feedback rule sends past it, see launch_batch)
// and can take the gate-less FIXED loop of gs_match_kernel takes it if the same predicted pass probability is below
// GS_PF_NOGATE_MAX_PASS.  The survivors of such a store are nearly all reads from the store, for which the minimizer gate passes
// nearly every lane; the background reads that survive pay for the record lines the gate would have kept them from, so the bound is
// HALF the break-even pass rate of a half-and-half stream, Δg / Δb ("Survivors skip the gate", has both figures and the
// arithmetic).  mode is GS_PF_GATE, read per run like GS_PREFILTER: 1 keeps the gate, 0 drops it for every FIXED batch that can take
// the loop, anything else leaves it to the rule.
#define GS_PF_NOGATE_MAX_PASS 0.2
extern "C" int gs_match_gate_rule(int64_t n_lmers, int samples, int mode, double *predicted_pass) {
    const double pass = prefilter_pass(n_lmers, samples);
    if (predicted_pass) *predicted_pass = pass;
    if (mode == 0 || mode == 1) return mode == 0 ? 1 : 0;
    return pass < GS_PF_NOGATE_MAX_PASS ? 1 : 0;
}
static bool prefilter_eligible(const gs_db *db) { return db->d_rec != nullptr && !db->striped() && db->n_parts <= 1 && db->info.k >= GS_MIN_K; }

// builds the filter of a store that has none yet: one sweep over the record lines and the table, then the popcount of the exact level
static int db_ensure_prefilter(gs_db *db, int mode) {
    if (mode == 0 || db->pf_set >= 0 || !prefilter_eligible(db)) return GS_OK;
    const size_t l1_words = (size_t)1 << (GS_PF_L1_BITS - 5);
    hipStream_t stream = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    u64 *d_count = nullptr;
    u64 count = 0;
    hipError_t e = gs_dev_alloc((void **)&db->d_pf, sizeof(uint32_t) * (GS_PF_L2_WORDS + l1_words));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&d_count, sizeof(u64));
    if (e == hipSuccess) e = hipMemsetAsync(db->d_pf, 0, sizeof(uint32_t) * (GS_PF_L2_WORDS + l1_words), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, sizeof(u64), stream);
    if (e == hipSuccess) {
        GsPrefilterBuildParams B{};
        B.rec = db->d_rec;
        B.n_rec = db->n_rec;
        B.tab = db->d_table;
        B.n_tab = db->info.n_buckets;
        B.bucket_bits = db->dev.bucket_bits;
        B.vbits = db->dev.vbits;
        B.k = db->info.k;
        B.l2 = db->d_pf;
        B.l1 = db->d_pf + GS_PF_L2_WORDS;
        B.count = (unsigned long long *)d_count;
        e = gs_launch_prefilter_build(&B, db->n_cu, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&count, d_count, sizeof(u64), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    gs_dev_free(d_count);
    hipStreamDestroy(stream);
    if (e != hipSuccess) {
        gs_dev_free(db->d_pf);
        db->d_pf = nullptr;
        return hip_fail(e, "prefilter build");
    }
    db->pf_set = (int64_t)count;
    // a store too dense for the rule at the fewest samples a batch can have (L = 128) keeps |S| and gives the memory back
    if (!prefilter_rule(db, mode, gs_pf_samples(128, db->info.k))) {
        gs_dev_free(db->d_pf);
        db->d_pf = nullptr;
    }
    return GS_OK;
}

extern "C" int gs_match_begin(gs_run **out, gs_db *db, const gs_match_cfg *cfg) {
    if (!out || !db || !cfg) return fail(GS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (cfg->max_paths < 1 || cfg->max_paths > 128) return fail(GS_E_INVALID, "max_paths must be in [1,128] (C/GSConfigKey.java:350)");
    HIP_TRY(hipSetDevice(db->device));
    if (!db->complete()) return fail(GS_E_STATE, "striped store: not every stripe is attached yet (gs_db_stripe_attach)");
    if (cfg->count_unique && db->unique_owner && !db->striped())
        return fail(GS_E_STATE, "this store already has an active unique-counting run (the seen bits live in the table)");
    int pf_mode = -1;
    if (const char *ev = getenv("GS_PREFILTER")) pf_mode = atoi(ev) != 0 ? 1 : 0;
    {
        const int prc = db_ensure_prefilter(db, pf_mode);
        if (prc) return prc;
    }
    gs_run *run = new gs_run();
    run->db = db;
    run->cfg = *cfg;
    run->pf_mode = pf_mode;
    if (const char *ev = getenv("GS_PF_GATE")) run->gate_mode = atoi(ev) != 0 ? 1 : 0;
    if (const char *ev = getenv("GS_SN_DEFER")) run->sn_mode = atoi(ev) != 0 ? 1 : 0;
    const size_t nv = (size_t)db->info.n_values;
    run->bitmap_words = (db->n_slots() + 31) / 32 + db->n_rec;  // one word per record bucket behind the table slots' bits
    hipError_t e = hipStreamCreateWithFlags(&run->stream, hipStreamNonBlocking);
    // Counters that do not fit the LDS are global atomics: 12 bytes x 8 per tax id in three cache lines that every CU
    // hits.  Measured on the 47 M-k-mer / 526-value store: they cost 8 of 16.7 ms on reads from the store; spread over
    // 16 copies (one per group of workgroups) the lines are 16 times colder.
    // (developer knob, see gs_launch_match: the launchers cache it once per process, this reads it per run -- set it before the
    // process starts, never in between)
    const char *force_global = getenv("GS_FORCE_GLOBAL_STATS");
    if (nv > GS_NV_LDS || (force_global != nullptr && atoi(force_global) != 0)) {
        int copies = 16;
        if (const char *ev = getenv("GS_STAT_COPIES")) copies = std::max(1, std::min(64, atoi(ev)));
        while (copies > 1 && (size_t)copies * nv * 96 > ((size_t)64 << 20)) copies /= 2;
        run->stat_copies = copies;
        // and most reads need no atomics at all: the hit k-mers of a read usually carry one tax id, whose statistics go
        // into one 64-byte record per read that a second kernel adds up in LDS (gs_stat_reduce_kernel)
        run->use_stat_recs = nv <= GS_STAT_REC_MAX_VALUES;
        if (const char *ev = getenv("GS_STAT_RECS")) run->use_stat_recs = run->use_stat_recs && atoi(ev) != 0;
    }
    else {
        // counters in LDS: every workgroup adds its table to the device's when it ends -- 2 048 workgroups x the same few cache lines,
        // and atomics on one line execute one after the other (~11 ns each: a tail of 0.1-0.2 ms behind the kernel).  16 copies here too.
        run->stat_copies = 16;
        if (const char *ev = getenv("GS_STAT_COPIES")) run->stat_copies = std::max(1, std::min(64, atoi(ev)));
        run->sn_lds = true;
    }
    const size_t cp = (size_t)run->stat_copies;
    // sums | max keys | double sums | long-read queue counters in ONE allocation: one memset clears them (gs_match_reset)
    if (e == hipSuccess) e = gs_dev_alloc((void **)&run->d_sums, sizeof(int64_t) * nv * (GS_N_SUMS + 1 + GS_N_DCOLS) * cp + GS_QUEUE_WORDS * sizeof(unsigned int));
    if (e == hipSuccess) {
        run->d_max = run->d_sums + nv * GS_N_SUMS * cp;
        run->d_dsums = reinterpret_cast<double *>(run->d_max + nv * cp);
        run->d_long_count = reinterpret_cast<unsigned int *>(run->d_dsums + nv * GS_N_DCOLS * cp);
    }
    if (e == hipSuccess) e = gs_dev_alloc((void **)&run->d_bitmap, sizeof(uint32_t) * (size_t)run->bitmap_words);
    if (e == hipSuccess && !db->striped())  // (run_clear clears a striped store's bitmap, and no other)
        e = hipMemsetAsync(run->d_bitmap, 0, sizeof(uint32_t) * (size_t)run->bitmap_words, run->stream);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&run->d_result, sizeof(u64) * nv * (GS_N_SUMS + 2 + GS_N_DCOLS));
    if (e == hipSuccess) run->d_unique = run->d_result + nv * (GS_N_SUMS + 1);
    if (e == hipSuccess && cfg->max_kmer_res_counts > 0)
        e = gs_dev_alloc((void **)&run->d_hit_counts, sizeof(uint32_t) * (size_t)(db->n_slots() + db->n_rec * GS_REC_SLOTS));
    if (e != hipSuccess) {
        run_free(run);
        return hip_fail(e, "run alloc");
    }
    int occ = gs_match_occupancy(db->info.n_values);
    if (occ < 1) occ = 1;
    if (occ > 8) occ = 8;  // 8 workgroups (32 waves) per CU: the kernel is built for 64 VGPRs
    if (const char *ev = getenv("GS_MATCH_BLOCKS_PER_CU")) {
        int v = atoi(ev);
        if (v >= 1 && v <= 16) occ = v;
    }
    run->grid = db->n_cu * occ;
    run->seen_dirty = cfg->count_unique != 0;  // a previous owner may have left seen bits behind
    int rc = run_clear(run);
    if (rc) {
        run_free(run);
        return rc;
    }
    if (cfg->count_unique && !db->striped()) db->unique_owner = run;  // (a striped store is read-only: any number of runs)
    db->live_runs++;
    *out = run;
    return GS_OK;
}

static int ensure_long(gs_run *run, int64_t n_reads) {
    // (the queue is filled in chunks of 64 entries per wave of the match kernel: every wave may leave one partly used)
    const int64_t room = n_reads + (int64_t)run->grid * (GS_BLOCK / 64) * 64;
    if (run->long_cap < room) {  // (three queues: long reads, reads for the three- and the four-sub-round kernel)
        HIP_TRY(hipStreamSynchronize(run->stream));
        gs_dev_free(run->d_long_list);
        run->d_long_list = nullptr;
        run->long_cap = 0;
        int64_t cap = std::max<int64_t>(room, 1024);
        HIP_TRY(gs_dev_alloc((void **)&run->d_long_list, sizeof(uint32_t) * (size_t)cap * 3));
        run->long_cap = cap;
    }
    if (!run->d_scratch) {
        // (where the longest reads leave the one-wave path, gs_match_huge_kernel: tunables and test hooks)
        if (const char *e = getenv("GS_HUGE_MIN")) run->huge_min = std::max(129, atoi(e));
        if (const char *e = getenv("GS_HUGE_CHUNK")) run->huge_chunk_min = std::max(128, (atoi(e) + 127) & ~127);
        // long-read kernel: a persistent grid that fills the device (the widest variant's occupancy; one wave per SIMD ran
        // 7-16x below the short-read kernel's rate per base), each wave owns tag[n_values] + cnt[n_values] in HBM
        const size_t nv = (size_t)run->db->info.n_values;
        int occ = gs_match_long_occupancy((int)nv);
        if (occ < 1) occ = 1;
        if (occ > 8) occ = 8;
        if (const char *e = getenv("GS_LONG_BLOCKS_PER_CU")) {
            const int v = atoi(e);
            if (v >= 1 && v <= 8) occ = v;
        }
        int grid = run->db->n_cu * occ;
        while (grid > 8 && (size_t)grid * 4 * nv * 2 * sizeof(int32_t) > ((size_t)2 << 30)) grid /= 2;
        run->long_grid = grid;
        const size_t waves = (size_t)grid * (GS_BLOCK / 64);
        HIP_TRY(gs_dev_alloc((void **)&run->d_scratch, waves * nv * 2 * sizeof(int32_t)));
        HIP_TRY(gs_dev_alloc((void **)&run->d_serial, waves * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(run->d_scratch, 0, waves * nv * 2 * sizeof(int32_t), run->stream));
        HIP_TRY(hipMemsetAsync(run->d_serial, 0, waves * sizeof(uint32_t), run->stream));
        if (const char *e = getenv("GS_TEST_LONG_SERIAL")) {
            // test hook for the serial wrap of gs_match_long_kernel: start every wave's serial just below 2^32 and fill
            // its tag / count rows with the values the serials take right after the wrap (1, 2, ..): without the clear
            // on wrap the first reads after it would take stale tags for their own
            const unsigned long v = strtoul(e, nullptr, 0);
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)run->d_serial, (int)(uint32_t)v, waves, run->stream));
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)run->d_scratch, 1, waves * nv * 2, run->stream));
        }
    }
    return GS_OK;
}

// the rows of the huge-read kernels; they leave them clean (gs_match_huge_finish_kernel), so this runs once per run
static int ensure_huge(gs_run *run, GsMatchParams *P) {
    const size_t nv = (size_t)run->db->info.n_values;
    const size_t per_slot_words = (3 * (size_t)GS_HUGE_COPIES + 2) * nv;  // votes, first positions, touch list per copy + the folded pair
    if (!run->d_huge) {
        int slots = (int)std::min<size_t>(GS_HUGE_SLOTS, std::max<size_t>(4, ((size_t)256 << 20) / (per_slot_words * 4)));
        if (const char *e = getenv("GS_HUGE_SLOTS")) slots = std::max(1, std::min(GS_HUGE_SLOTS, atoi(e)));
        const size_t fixed = 16 + sizeof(uint32_t) * GS_HUGE_SLOTS + sizeof(GsHugeHead) * GS_HUGE_SLOTS * GS_HUGE_COPIES;
        const size_t chunks = sizeof(GsHugeChunk) * (size_t)slots * GS_HUGE_MAX_CHUNKS, row = sizeof(uint32_t) * (size_t)slots * GS_HUGE_COPIES * nv;
        const size_t fold = sizeof(uint32_t) * (size_t)slots * 2 * nv;
        HIP_TRY(gs_dev_alloc((void **)&run->d_huge, fixed + chunks + 3 * row + fold));
        HIP_TRY(hipMemsetAsync(run->d_huge, 0, fixed + chunks + row, run->stream));
        HIP_TRY(hipMemsetAsync(run->d_huge + fixed + chunks + row, 0xff, row, run->stream));  // first positions: none
        HIP_TRY(hipMemsetAsync(run->d_huge + fixed + chunks + 3 * row, 0, fold, run->stream));
        run->huge_slots = slots;
    }
    const size_t slots = (size_t)run->huge_slots;
    unsigned char *p = run->d_huge;
    P->huge_count = reinterpret_cast<unsigned int *>(p);
    p += 16;
    P->huge_list = reinterpret_cast<uint32_t *>(p);
    p += sizeof(uint32_t) * GS_HUGE_SLOTS;
    P->huge_head = reinterpret_cast<GsHugeHead *>(p);
    p += sizeof(GsHugeHead) * GS_HUGE_SLOTS * GS_HUGE_COPIES;
    P->huge_chunks = reinterpret_cast<GsHugeChunk *>(p);
    p += sizeof(GsHugeChunk) * slots * GS_HUGE_MAX_CHUNKS;
    P->huge_cnt = reinterpret_cast<uint32_t *>(p);
    p += sizeof(uint32_t) * slots * GS_HUGE_COPIES * nv;
    P->huge_first = reinterpret_cast<uint32_t *>(p);
    p += sizeof(uint32_t) * slots * GS_HUGE_COPIES * nv;
    P->huge_touch = reinterpret_cast<uint32_t *>(p);
    p += sizeof(uint32_t) * slots * GS_HUGE_COPIES * nv;
    P->huge_fold = reinterpret_cast<uint32_t *>(p);
    P->huge_slots = run->huge_slots;
    P->huge_min = run->huge_min;
    P->huge_chunk_min = run->huge_chunk_min;
    return hipMemsetAsync(P->huge_count, 0, sizeof(unsigned int), run->stream) == hipSuccess ? GS_OK : fail(GS_E_HIP, "huge-read counter");
}

// The table of a batch of one read length with `max` k-mer positions (65 .. 128: what the FIXED loop of gs_match_kernel takes), keyed
// by max and the run's two gate settings; every predicate and quotient is the general loop's expression (gs_process_read),
// evaluated here for every error count the length allows.  One upload per change of length, on
// the run's stream and from memory the run owns: batches of the same length copy nothing.
static int ensure_quot(gs_run *run, int max) {
    const double m = run->cfg.max_read_tax_err, mc = run->cfg.max_read_class_err;
    if (run->quot_max == max && run->quot_tax == m && run->quot_class == mc) return GS_OK;
    if (!run->d_quot) {
        HIP_TRY(gs_dev_alloc((void **)&run->d_quot, sizeof(GsQuotTable)));
        HIP_TRY(hipHostMalloc((void **)&run->h_quot, sizeof(GsQuotTable), hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&run->quot_copied, hipEventDisableTiming));
    } else
        HIP_TRY(hipEventSynchronize(run->quot_copied));  // (the previous length's upload reads h_quot)
    run->quot_max = 0;
    GsQuotTable &T = *run->h_quot;
    memset(&T, 0, sizeof(T));
    for (int i = 0; i <= max; i++) {
        const int tax_err = i, class_err = i;
        const double q = (double)i / (double)max;
        T.e[i].q = q;
        T.e[i].q2 = q * q;
        const bool disabled = m >= 0 && ((m >= 1 && (double)tax_err > m) || ((double)tax_err > m * (double)max));
        const bool counted = mc < 0 || (mc >= 1 && (double)class_err <= mc) || ((double)class_err <= mc * (double)max);
        if (disabled) T.tax_disabled[i >> 5] |= 1u << (i & 31);
        if (counted) T.class_counted[i >> 5] |= 1u << (i & 31);
    }
    HIP_TRY(hipMemcpyAsync(run->d_quot, run->h_quot, sizeof(GsQuotTable), hipMemcpyHostToDevice, run->stream));
    HIP_TRY(hipEventRecord(run->quot_copied, run->stream));
    run->quot_max = max;
    run->quot_tax = m;
    run->quot_class = mc;
    return GS_OK;
}

static int launch_batch(gs_run *run, const uint8_t *d_seq, const uint64_t *d_off, int64_t n_reads, int64_t first_read_no,
                        int32_t *d_class, uint8_t *d_flags, const int32_t *d_nodes = nullptr,
                        const uint64_t *d_pos_off = nullptr, int off_stride = 1, const uint32_t *d_skip = nullptr, int fixed_len = 0) {
    if (n_reads > (int64_t)0xffffffffLL) return fail(GS_E_INVALID, "more than 2^32-1 reads in one batch");
    int rc = ensure_long(run, n_reads);
    if (rc) return rc;
    GsMatchParams P{};
    P.db = run->db->dev;
    P.seq = d_seq;
    P.off = d_off;
    P.n_reads = n_reads;
    P.first_read_no = first_read_no;
    P.classify = run->cfg.classify;
    P.count_unique = run->cfg.count_unique;
    P.max_paths = run->cfg.max_paths;
    P.threshold = run->cfg.threshold;
    P.max_read_tax_err = run->cfg.max_read_tax_err;
    P.max_read_class_err = run->cfg.max_read_class_err;
    P.sums = run->d_sums;
    P.max_keys = run->d_max;
    P.dsums = run->d_dsums;
    P.stat_copies = run->stat_copies;
    run->stats_spread = run->stat_copies > 1;
    P.bitmap = run->d_bitmap;
    P.hit_counts = run->d_hit_counts;
    P.class_vi = d_class;
    P.flags = d_flags;
    P.long_count = run->d_long_count;
    P.long_list = run->d_long_list;
    P.long_cap = run->long_cap;
    P.nodes = d_nodes;
    P.pos_off = (const unsigned long long *)d_pos_off;
    P.off_stride = off_stride;
    P.fixed_len = fixed_len;
    P.skip = d_skip;
    // (the batches whose waves take the FIXED loop of gs_match_kernel, and no others, need the table; that loop takes none without it)
    if (off_stride == 0 && !d_nodes && fixed_len >= 128 && fixed_len - run->db->info.k + 1 <= GS_QUOT_ENTRIES - 1) {
        if ((rc = ensure_quot(run, fixed_len - run->db->info.k + 1))) return rc;
        P.quot = run->d_quot;
    }
    int grid = (int)std::min<int64_t>(run->grid, (n_reads + (GS_BLOCK / 64) - 1) / (GS_BLOCK / 64));
    if (grid < 1) grid = 1;
    const int64_t rec_room = n_reads + (int64_t)grid * (GS_BLOCK / 64) * 64;  // every wave may leave one chunk of 64 partly used
    if (run->use_stat_recs) {
        if ((rc = grow(&run->d_stat_recs, &run->stat_recs_cap, (size_t)rec_room, run->stream))) return rc;
        /* (640 = GS_REDUCE_VALUES, the values one pass of gs_stat_reduce_kernel takes) */
        if (run->db->info.n_values > 640 && (rc = grow(&run->d_stat_vi, &run->stat_vi_cap, (size_t)rec_room, run->stream))) return rc;
        if (!run->d_stat_rec_count) HIP_TRY(gs_dev_alloc((void **)&run->d_stat_rec_count, sizeof(u64)));
        HIP_TRY(hipMemsetAsync(run->d_stat_rec_count, 0, sizeof(u64), run->stream));
        P.stat_recs = run->d_stat_recs;
        P.stat_rec_count = (unsigned long long *)run->d_stat_rec_count;
    }
    // Reads of one length with at most 128 k-mer positions, not from nodes: gs_classify_kernel does not run, and it alone writes the
    // queues of the wide and the long-read kernels -- which return at once on an empty queue and keep nothing else from launch to
    // launch (the cursors and queue lengths are cleared right here by every batch that launches them, the long-read kernel's
    // serials move only with a read it takes).  So such a batch launches none of them and leaves the queue counters alone.
    // (reads of one short length each, or nodes that came from other ranks: nothing for the huge-read kernels)
    const bool huge = !d_nodes && (off_stride != 0 || fixed_len - run->db->info.k + 1 >= run->huge_min);
    const bool no_queues = off_stride == 0 && !d_nodes && fixed_len - run->db->info.k + 1 <= 128 && !huge;
    if (!no_queues) HIP_TRY(hipMemsetAsync(run->d_long_count, 0, 6 * sizeof(unsigned int), run->stream));
    if (huge && (rc = ensure_huge(run, &P))) return rc;
    // The batches of the FIXED loop, and only those, may go through the prefilter first: the match kernel then takes the survivors
    // from the list (queue 0 of the long-read list, which such a batch does not use) and their number from the word behind the queue
    // counters.  Results do not depend on which way a batch goes.
    run->pf_last_survivors = -1;
    run->pf_last_reads = n_reads;
    run->pf_last_slot = -1;
    bool prefilter = P.quot != nullptr && fixed_len - run->db->info.k + 1 >= 65 && !d_skip && no_queues &&
                     prefilter_rule(run->db, run->pf_mode, gs_pf_samples(fixed_len, run->db->info.k));
    bool paused = false;  // the rule sends this store's batches through the prefilter, the feedback rule sends this one past it
    if (prefilter && run->pf_mode < 0) {  // the feedback rule (a forced prefilter is not paused)
        for (int i = 0; i < GS_PF_SLOTS; i++)
            if (run->pf_slot_pending[i] && run->pf_h[i] != 0xffffffffu) {
                run->pf_slot_pending[i] = false;
                if ((double)run->pf_h[i] > GS_PF_HIT_RICH * (double)run->pf_slot_reads[i]) run->pf_pause = GS_PF_PAUSE;
            }
        if (run->pf_pause > 0) {
            run->pf_pause--;
            prefilter = false;
            paused = true;
        }
    }
    // The batches whose waves take the FIXED loop of gs_match_kernel<true, ..> (counters in LDS, one candidate path per lane, one
    // store): every read goes out as a record or a row of node codes.  Without room for them the batch takes the general loop.
    run->sn_last = false;
    if (P.quot != nullptr && run->sn_lds && run->sn_mode != 0 && run->cfg.max_paths <= 64 && P.db.n_parts <= 1 && !d_skip &&
        P.db.n_values <= GS_SN_CODE_MAX && grow(&run->d_sn_recs, &run->sn_recs_cap, (size_t)n_reads, run->stream) == GS_OK &&
        grow(&run->d_sn_list, &run->sn_list_cap, (size_t)n_reads, run->stream) == GS_OK &&
        grow(&run->d_sn_nodes, &run->sn_nodes_cap, (size_t)n_reads * GS_SN_ROW, run->stream) == GS_OK) {
        P.sn_recs = run->d_sn_recs;
        P.sn_nodes = run->d_sn_nodes;
        run->sn_last = true;
    }
    // The gate rule (above prefilter_rule's neighbours): only a batch whose waves take the FIXED loop of the one-store, 64-path
    // kernels whose gate is keyed by the minimizer alone, on a store with a gate and records, can drop the gate (gs_launch_match
    // refuses the flag anywhere else).  A paused batch is, by the evidence that paused the prefilter, one the gate does nothing for.
    run->gate_last_gateless = false;
    run->gate_last_pass = -1.0;
    if (P.quot != nullptr && !d_nodes && !d_skip && P.db.n_parts <= 1 && run->cfg.max_paths <= 64 && !P.db.mgate_ctx &&
        P.db.mgate != nullptr && P.db.rec != nullptr && prefilter_eligible(run->db) && (!run->sn_lds || P.sn_recs != nullptr)) {
        const int gateless = gs_match_gate_rule(run->db->pf_set, gs_pf_samples(fixed_len, run->db->info.k), run->gate_mode, &run->gate_last_pass);
        run->gate_last_gateless = gateless != 0 && (run->gate_mode == 0 || prefilter || paused);
        P.fixed_nogate = run->gate_last_gateless ? 1 : 0;
    }
    int pf_slot = -1;
    if (prefilter) {
        if (!run->pf_h) {
            HIP_TRY(hipHostMalloc((void **)&run->pf_h, sizeof(uint32_t) * GS_PF_SLOTS, hipHostMallocDefault));
            for (int i = 0; i < GS_PF_SLOTS; i++) run->pf_h[i] = 0;
        }
    }
    // (word 6 behind the queue counters: the survivors; word 7: the records booked; word 8: the rows of node codes listed.  One
    // memset for all)
    if (prefilter || P.sn_recs)
        HIP_TRY(hipMemsetAsync(run->d_long_count + (prefilter ? 6 : 7), 0, sizeof(unsigned int) * ((prefilter ? 1 : 0) + (P.sn_recs ? 2 : 0)), run->stream));
    if ((rc = timer_start(run->timer, run->cfg.profile != 0, run->stream))) return rc;
    if (prefilter) {
        GsPrefilterParams F{};
        F.seq = d_seq;
        F.n_reads = n_reads;
        F.L = fixed_len;
        F.k = run->db->info.k;
        F.l2 = run->db->d_pf;
        F.l1 = run->db->d_pf + GS_PF_L2_WORDS;
        F.list = run->d_long_list;
        F.count = run->d_long_count + 6;
        F.class_vi = d_class;
        F.flags = d_flags;
        HIP_TRY(gs_launch_prefilter(&F, run->stream));
        P.surv_list = run->d_long_list;
        P.surv_count = run->d_long_count + 6;
        pf_slot = (int)(run->pf_batches % GS_PF_SLOTS);
        if (run->pf_slot_pending[pf_slot] && run->pf_h[pf_slot] == 0xffffffffu) pf_slot = -1;  // (its copy of four batches ago is still under way)
    }
    if (run->cfg.count_unique && !d_nodes) {
        run->seen_dirty = true;
        run->bitmap_merged = false;
    }
    // reads of one length with more than 128 k-mer positions (250-bp pairs, 150 bp at k < 23): every one of them would be queued for the
    // long-read kernel -- the pass that queues them is skipped (2.0 of 16.2 ms for 10 M reads of 150 bp at k = 16), the queue is the batch
    const bool all_long = off_stride == 0 && !d_nodes && !d_skip && fixed_len - run->db->info.k + 1 > 128 && !huge;
    static const bool wide_on = !getenv("GS_WIDE") || atoi(getenv("GS_WIDE")) != 0;  // (GS_WIDE=0: every read above 128 positions on the long-read path)
    P.wide_mask = wide_on ? gs_match_wide_mask(&P) : 0;
    if (all_long)
        P.long_list = nullptr;
    else {
        // reads of more than 128 positions into the queues of the kernels that take them (reads of one short length: there are none)
        if (off_stride != 0 || fixed_len - run->db->info.k + 1 > 128) HIP_TRY(gs_launch_classify(&P, run->stream));
        HIP_TRY(gs_launch_match(&P, grid, run->stream));
        if (P.sn_recs) {  // (part of the timed region, as the deferred statistics below)
            GsSnReduceParams S{};
            S.recs = P.sn_recs;
            S.count = P.surv_count;
            S.n_reads = n_reads;
            S.first_read_no = first_read_no;
            S.c.max = fixed_len - run->db->info.k + 1;
            S.c.read_len = fixed_len;
            S.c.classify = P.classify;
            S.c.threshold = P.threshold;
            S.n_values = P.db.n_values;
            S.stat_copies = P.stat_copies;
            S.quot = P.quot;
            S.sums = P.sums;
            S.max_keys = P.max_keys;
            S.dsums = P.dsums;
            S.class_vi = d_class;
            S.flags = d_flags;
            S.booked = run->d_long_count + 7;
            S.row_list = run->d_sn_list;
            S.n_rows = run->d_long_count + 8;
            S.nodes = P.sn_nodes;
            S.parent = P.db.parent;
            S.tin = P.db.tin;
            S.tout = P.db.tout;
            S.max_paths = P.max_paths;
            HIP_TRY(gs_launch_sn_reduce(&S, run->stream));
        }
    }
    if (P.stat_recs && !all_long)  // (into copy 0 of the counters; part of the timed region)
        HIP_TRY(gs_launch_stat_reduce(P.stat_recs, run->d_stat_rec_count, rec_room, run->db->info.n_values, run->d_sums, run->d_max,
                                      run->d_dsums, run->d_stat_vi, run->stream));
    if ((rc = timer_stop(run->timer, run->cfg.profile != 0, run->stream))) return rc;
    if (prefilter) {
        run->pf_batches++;
        run->pf_last_survivors = 0;  // (known once the batch is through: gs_match_prefilter_info)
        if (pf_slot >= 0) {
            run->pf_h[pf_slot] = 0xffffffffu;
            run->pf_slot_reads[pf_slot] = n_reads;
            run->pf_slot_pending[pf_slot] = true;
            run->pf_last_slot = pf_slot;
            HIP_TRY(hipMemcpyAsync(run->pf_h + pf_slot, run->d_long_count + 6, sizeof(uint32_t), hipMemcpyDeviceToHost, run->stream));
        }
    }
    const int pos_fixed = fixed_len - run->db->info.k + 1;
    if (all_long && pos_fixed <= 256 && ((P.wide_mask >> (pos_fixed <= 192 ? 0 : 1)) & 1)) {  // the whole batch in trips of three / four sub-rounds
        HIP_TRY(gs_launch_match_wide(&P, pos_fixed <= 192 ? 3 : 4, run->db->n_cu, run->stream));
        return GS_OK;
    }
    if (no_queues) return GS_OK;
    if (!all_long && P.wide_mask) {  // what gs_match_kernel put into queues 1 and 2 (the kernels return at once when their queue is empty)
        if (P.wide_mask & 1) HIP_TRY(gs_launch_match_wide(&P, 3, run->db->n_cu, run->stream));
        if (P.wide_mask & 2) HIP_TRY(gs_launch_match_wide(&P, 4, run->db->n_cu, run->stream));
    }
    // reads with more than 128 k-mer positions were queued; the long-read kernel drains the queue
    HIP_TRY(gs_launch_match_long(&P, run->long_grid, run->d_scratch, run->d_serial, run->stream));
    if (huge) HIP_TRY(gs_launch_match_huge(&P, run->long_grid, run->stream));  // ... and hands the longest ones on
    return GS_OK;
}

extern "C" int gs_match_submit(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                               int64_t first_read_no, int mem, int32_t *class_vi, uint8_t *flags) try {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    if (n_reads < 0 || (n_reads > 0 && (!seq || !offsets))) return fail(GS_E_INVALID, "bad batch arrays");
    if (n_reads == 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    if (mem == GS_MEM_DEVICE) return launch_batch(run, seq, offsets, n_reads, first_read_no, class_vi, flags);
    if (mem != GS_MEM_HOST) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    // host batch: stage to HBM (synchronous)
    HostStage &h = run->host;
    int rc = stage_room(h, (size_t)(offsets[n_reads] - offsets[0]), (size_t)n_reads, run->stream);
    if (!rc) rc = stage_upload(h, seq, offsets, n_reads, run->stream);
    if (!rc) rc = launch_batch(run, h.d_seq, h.d_off, n_reads, first_read_no, class_vi ? h.d_class : nullptr, flags ? h.d_flags : nullptr);
    if (!rc) rc = stage_download(h, class_vi, flags, n_reads, run->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(run->stream));
    return timer_collect(run->timer);
}
GS_API_CATCH

// reads of ONE length, back to back, without an offsets array (what a sequencer's FASTQ gives once parsed: `read_len` bases each)
extern "C" int gs_match_submit_fixed(gs_run *run, const uint8_t *seq, int32_t read_len, int64_t n_reads, int64_t first_read_no, int mem,
                                     int32_t *class_vi, uint8_t *flags) try {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    if (n_reads < 0 || read_len < 0 || (n_reads > 0 && !seq)) return fail(GS_E_INVALID, "bad batch arrays");
    if (n_reads == 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    if (mem == GS_MEM_DEVICE)
        return launch_batch(run, seq, nullptr, n_reads, first_read_no, class_vi, flags, nullptr, nullptr, 0, nullptr, read_len);
    if (mem != GS_MEM_HOST) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HostStage &h = run->host;
    const size_t nbytes = (size_t)n_reads * (size_t)read_len;
    int rc = stage_room(h, nbytes, (size_t)n_reads, run->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h.d_seq, seq, nbytes, hipMemcpyHostToDevice, run->stream));  // (no offsets: nothing to rebase)
    rc = launch_batch(run, h.d_seq, nullptr, n_reads, first_read_no, class_vi ? h.d_class : nullptr, flags ? h.d_flags : nullptr, nullptr, nullptr,
                      0, nullptr, read_len);
    if (!rc) rc = stage_download(h, class_vi, flags, n_reads, run->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(run->stream));
    return timer_collect(run->timer);
}
GS_API_CATCH

// the asynchronous form of a host batch: returns when the work is queued; gs_match_wait(ticket) returns when the
// batch's per-read outputs are in place and its input arrays may be reused.  Two batches can be under way.
extern "C" int gs_match_submit_async(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                                     int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket) try {
    if (!run || !ticket) return fail(GS_E_INVALID, "NULL argument");
    if (n_reads <= 0 || !seq || !offsets) return fail(GS_E_INVALID, "bad batch arrays");
    HIP_TRY(hipSetDevice(run->db->device));
    BatchStage &g = run->stage;
    if (!g.copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&g.copy_stream, hipStreamNonBlocking));
        for (hipEvent_t &ev : g.copied) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (hipEvent_t &ev : g.finished) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const int64_t tk = g.tickets;
    const int b = (int)(tk & 1);
    HostStage &h = g.bank[b];
    if (tk >= 2) HIP_TRY(hipEventSynchronize(g.copied[b]));  // h.rel of the batch before last is free (long done)
    int rc = stage_room(h, (size_t)(offsets[n_reads] - offsets[0]), (size_t)n_reads, run->stream, g.copy_stream);
    if (rc) return rc;
    // the batch before last must be through (its kernel read these buffers, its outputs left from them).  Waited for
    // on the host: a copy that has to wait for an event on the device was seen to start only after the kernel of the
    // previous batch had ended (rocprofv3 --memory-copy-trace), i.e. not to overlap at all
    if (tk >= 2) HIP_TRY(hipEventSynchronize(g.finished[(tk - 2) & 3]));
    if ((rc = stage_upload(h, seq, offsets, n_reads, g.copy_stream))) return rc;
    HIP_TRY(hipEventRecord(g.copied[b], g.copy_stream));
    HIP_TRY(hipStreamWaitEvent(run->stream, g.copied[b], 0));
    rc = launch_batch(run, h.d_seq, h.d_off, n_reads, first_read_no, class_vi ? h.d_class : nullptr, flags ? h.d_flags : nullptr);
    if (!rc) rc = stage_download(h, class_vi, flags, n_reads, run->stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(g.finished[tk & 3], run->stream));
    g.tickets = tk + 1;
    *ticket = tk;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_match_wait(gs_run *run, int64_t ticket) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    BatchStage &g = run->stage;
    if (ticket < 0 || ticket >= g.tickets) return fail(GS_E_INVALID, "unknown ticket");
    HIP_TRY(hipSetDevice(run->db->device));
    // (a batch three or more behind the latest is through: the submit of the batch two after it waited for it)
    if (ticket + 3 <= g.tickets) return GS_OK;
    HIP_TRY(hipEventSynchronize(g.finished[ticket & 3]));
    return GS_OK;
}

// ---- text mode: raw 4-line FASTQ chunks, records found on the device (gs_text.hip) ------------------------------
extern "C" int gs_pinned_alloc(void **p, size_t bytes) {
    if (!p) return fail(GS_E_INVALID, "NULL argument");
    *p = nullptr;
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
    return GS_OK;
}

extern "C" int gs_pinned_free(void *p) {
    if (p) HIP_TRY(hipHostFree(p));
    return GS_OK;
}

static int match_submit_text(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int64_t first_read_no,
                             int32_t *class_vi, uint8_t *flags, int64_t *ticket, int64_t fasta_records, int64_t *ml_out = nullptr);

extern "C" int gs_match_submit_fastq_ml(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int64_t first_read_no,
                                        int32_t *class_vi, uint8_t *flags, int64_t *n_records, int64_t *consumed_bytes, int64_t *consumed_lines,
                                        int64_t *ticket) try {
    if (!n_records || !consumed_bytes) return fail(GS_E_INVALID, "NULL argument");
    int64_t out[3] = {0, 0, 0};
    const int rc = match_submit_text(run, text, n_bytes, n_lines, mem, first_read_no, class_vi, flags, ticket, -1, out);
    return ml_report(rc, out, n_records, consumed_bytes, consumed_lines);
}
GS_API_CATCH

extern "C" int gs_match_submit_text(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem,
                                    int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket) try {
    return match_submit_text(run, text, n_bytes, n_lines, mem, first_read_no, class_vi, flags, ticket, -1);
}
GS_API_CATCH

extern "C" int gs_match_submit_fasta(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem,
                                     int64_t first_read_no, int32_t *class_vi, uint8_t *flags, int64_t *ticket) try {
    if (n_records < 0) return fail(GS_E_INVALID, "n_records < 0");
    return match_submit_text(run, text, n_bytes, n_lines, mem, first_read_no, class_vi, flags, ticket, n_records);
}
GS_API_CATCH

static int match_submit_text(gs_run *run, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, int64_t first_read_no,
                             int32_t *class_vi, uint8_t *flags, int64_t *ticket, int64_t fasta_records, int64_t *ml_out) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    TextBatch tb;
    int rc = text_batch(run->text, run->stream, text, n_bytes, n_lines, mem, run->db->info.k, ticket, fasta_records, ml_out, &tb);
    if (rc || tb.n_reads == 0) return rc;
    // host outputs land in the run's stage (its capacity is shared with the host batches: d_off grows with it)
    HostStage &h = run->host;
    if ((class_vi || flags) && !tb.dev_out && (rc = stage_room_reads(h, (size_t)tb.n_reads, run->stream))) return rc;
    int32_t *dc = class_vi ? (tb.dev_out ? class_vi : h.d_class) : nullptr;
    uint8_t *df = flags ? (tb.dev_out ? flags : h.d_flags) : nullptr;
    rc = launch_batch(run, tb.d_seq, (const uint64_t *)run->text.d_off2, tb.n_reads, first_read_no, dc, df, nullptr, nullptr, tb.off_stride, tb.d_skip);
    if (rc) return rc;
    if ((rc = text_touched(run->text, run->stream))) return rc;
    run->text.d_last_flags = df;
    run->text.d_last_class = dc;
    return tb.dev_out ? GS_OK : stage_download(h, class_vi, flags, tb.n_reads, run->stream);  // (complete after gs_match_sync)
}

// the reads matchRead() returned true for (GS_F_RETURNED), as afterMatch writes them (FastqKMerMatcher.java:304-307)
extern "C" int gs_match_compact_text(gs_run *run, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    return text_compact(run->text, run->stream, GS_F_RETURNED, 1, 1, slot, with_probs, d_out, n_bytes, n_records);
}

// the same for the records of a FASTA or general FASTQ chunk (gs_rewrite.hip)
extern "C" int gs_match_compact_records(gs_run *run, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) try {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    return text_records(run->text, run->stream, run->db->n_cu, GS_F_RETURNED, 1, 1, with_probs, slot, nullptr, false, d_out, n_bytes, n_records);
}
GS_API_CATCH

// the descriptor lines (whole first lines, '@' included) of a few records of the last four-line chunk: out[i * stride ..], NUL-terminated
extern "C" int gs_match_text_descriptors(gs_run *run, const int64_t *records, int32_t n, uint8_t *out, int32_t stride) {
    if (!run || n < 0 || (n > 0 && (!records || !out)) || stride < 2) return fail(GS_E_INVALID, "bad argument");
    if (n == 0) return GS_OK;
    TextScan &t = run->text;
    if (t.tickets == 0 || !t.last_four_line) return fail(GS_E_STATE, "the last chunk was not four-line FASTQ");
    for (int32_t i = 0; i < n; i++)
        if (records[i] < 0 || records[i] >= t.last_reads) return fail(GS_E_INVALID, "record outside the last chunk");
    HIP_TRY(hipSetDevice(run->db->device));
    int64_t *d_rec = nullptr;
    uint8_t *d_out = nullptr;
    hipError_t e = gs_dev_alloc((void **)&d_rec, sizeof(int64_t) * (size_t)n);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&d_out, (size_t)n * (size_t)stride);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rec, records, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, run->stream);
    int rc = GS_OK;
    if (e == hipSuccess && gs_gather_descriptors_device(run->stream, t.d_text, t.d_nl, d_rec, n, d_out, stride) != GS_OK) rc = fail(GS_E_HIP, gs_deflate_last_error());
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(out, d_out, (size_t)n * (size_t)stride, hipMemcpyDeviceToHost, run->stream);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(run->stream);
    gs_dev_free(d_rec);
    gs_dev_free(d_out);
    if (e != hipSuccess) return hip_fail(e, "gs_match_text_descriptors");
    return rc;
}

extern "C" int gs_match_text_wait_copy(gs_run *run, int64_t ticket) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    return text_wait_copy(run->text, ticket);
}

extern "C" int gs_match_text_status(gs_run *run, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    int rc = text_status(run->text, run->stream, failed_ticket, first_bad_record, totals);
    if (rc) return rc;
    return timer_collect(run->timer);
}

extern "C" int gs_match_text_select(gs_run *run, int bank) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    if (bank < 0 || bank >= GS_TEXT_BANKS) return fail(GS_E_INVALID, "text bank out of range");
    run->text.bank = bank;
    return GS_OK;
}

extern "C" int gs_match_text_clear_error(gs_run *run) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    return text_reset(run->text, false, run->stream);
}

// seen bits of the store -> the run's compact bitmap.  The kernels of a striped store write the bitmap themselves (the
// store's memory, partly another GPU's, is never written).
static int run_extract_bitmap(gs_run *run) {
    if (run->db->striped()) return GS_OK;
    HIP_TRY(gs_launch_bitmap_extract(run->db->d_table, run->db->n_slots(), run->d_bitmap, run->db->d_rec, run->db->n_rec, run->stream));
    run->bitmap_written = true;
    run->bitmap_stale = false;
    return GS_OK;
}

// before a read of the bitmap that no extract precedes: the bits that the last reset left in it (run_clear) go
static int bitmap_settle(gs_run *run) {
    if (!run->bitmap_stale) return GS_OK;
    HIP_TRY(hipMemsetAsync(run->d_bitmap, 0, sizeof(uint32_t) * (size_t)run->bitmap_words, run->stream));
    run->bitmap_stale = run->bitmap_written = false;
    return GS_OK;
}

// unique k-mers per value index from the bitmap (own or merged) into d_unique
static int run_unique_counts(gs_run *run) {
    const gs_db *db = run->db;
    HIP_TRY(hipMemsetAsync(run->d_unique, 0, sizeof(u64) * (size_t)db->info.n_values, run->stream));
    if (!db->striped()) {
        HIP_TRY(gs_launch_unique_count(db->d_table, run->d_bitmap, db->n_slots(), db->dev.vbits, db->info.n_values, run->d_unique,
                                       db->d_rec, db->n_rec, run->stream));
        return GS_OK;
    }
    // every stripe against its part of the bitmap (a foreign stripe is read over xGMI, once)
    const uint32_t *brec = run->d_bitmap + (db->n_slots() + 31) / 32;
    for (int q = 0; q < db->n_parts; q++) {
        int64_t tfirst = 0, tlocal = 0;
        const u64 *tq = stripe_table(db, q, &tfirst, &tlocal);
        HIP_TRY(gs_launch_unique_count(tq, run->d_bitmap + tfirst * GS_SLOTS_PER_BUCKET / 32, tlocal * GS_SLOTS_PER_BUCKET, db->dev.vbits,
                                       db->info.n_values, run->d_unique, nullptr, 0, run->stream));
        const int64_t first = (int64_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q);
        const int64_t local = (int64_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q + 1) - first;
        HIP_TRY(gs_launch_rec_unique_count(db->stripe_base[q], brec + first, local, db->info.n_values, run->d_unique, run->stream));
    }
    return GS_OK;
}

// the copies of the global-atomic counters into copy 0 (the others start from zero again)
// to_result (gs_match_finish): the totals also into d_result, its unique counts zeroed -- the same launch, also when there is
// nothing to fold
static int fold_stats(gs_run *run, bool to_result = false) {
    if (!run->stats_spread && !to_result) return GS_OK;
    HIP_TRY(gs_launch_fold_stats((long long *)run->d_sums, (unsigned long long *)run->d_max, run->d_dsums, (long long)run->db->info.n_values,
                                 run->stats_spread ? run->stat_copies : 1, to_result ? run->d_result : nullptr, run->stream));
    run->stats_spread = false;
    return GS_OK;
}

extern "C" int gs_match_get_device(gs_run *run, int *device) {
    if (!run || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = run->db->device;
    return GS_OK;
}

extern "C" int gs_match_sync(gs_run *run) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));
    return timer_collect(run->timer);
}

extern "C" int gs_match_finish(gs_run *run, int64_t *table, double *dtable) {
    if (!run || !table) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    const size_t nv = (size_t)run->db->info.n_values;
    // the result lands in page-locked memory (a copy into pageable memory is staged by the runtime: ~20 us, a third of the time
    // between two batches of the bench), and in ONE copy: the fold leaves the four arrays side by side in d_result
    if (!run->h_result) HIP_TRY(hipHostMalloc((void **)&run->h_result, sizeof(u64) * nv * (GS_N_SUMS + 2 + GS_N_DCOLS), hipHostMallocDefault));
    int64_t *sums = reinterpret_cast<int64_t *>(run->h_result);
    int64_t *maxk = sums + nv * GS_N_SUMS;
    u64 *uniq = reinterpret_cast<u64 *>(maxk + nv);
    double *dsums = reinterpret_cast<double *>(uniq + nv);
    {
        const int frc = fold_stats(run, true);
        if (frc) return frc;
    }
    if (run->cfg.count_unique) {
        const gs_db *db = run->db;
        if (!db->striped() && !run->bitmap_merged) {
            // the run's own seen bits: bitmap and counts in one pass over the store (d_unique: zeroed by the fold)
            HIP_TRY(gs_launch_seen_sweep(db->d_table, db->n_slots(), db->dev.vbits, db->d_rec, db->n_rec, run->d_bitmap, db->info.n_values,
                                         run->d_unique, run->stream));
            run->bitmap_written = true;
            run->bitmap_stale = false;
        } else {  // a merged bitmap, or the one that the kernels of a striped store write
            const int urc = run_unique_counts(run);
            if (urc) return urc;
        }
    }
    HIP_TRY(hipMemcpyAsync(run->h_result, run->d_result, sizeof(u64) * nv * (GS_N_SUMS + 2 + (dtable ? GS_N_DCOLS : 0)), hipMemcpyDeviceToHost,
                           run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    if (dtable) memcpy(dtable, dsums, sizeof(double) * nv * GS_N_DCOLS);
    int rc = timer_collect(run->timer);
    if (rc) return rc;
    for (size_t v = 0; v < nv; v++) {
        int64_t *row = table + v * GS_N_COLS;
        const int64_t *s = sums + v * GS_N_SUMS;
        row[GS_C_READS] = s[GS_S_READS];
        row[GS_C_READS_KMERS] = s[GS_S_READS_KMERS];
        row[GS_C_KMERS] = s[GS_S_KMERS];
        row[GS_C_UNIQUE_KMERS] = run->cfg.count_unique ? (int64_t)uniq[v] : -1;
        row[GS_C_CONTIGS] = s[GS_S_CONTIGS];
        row[GS_C_CONTIG_LEN_SQ_SUM] = s[GS_S_CONTIG_LEN_SQ_SUM];
        row[GS_C_READS_1KMER] = s[GS_S_READS_1KMER];
        row[GS_C_READS_BPS] = s[GS_S_READS_BPS];
        const u64 key = (u64)maxk[v];
        row[GS_C_MAX_CONTIG_LEN] = (int64_t)(key >> 40);
        row[GS_C_MAX_CONTIG_READ_NO] = key ? (int64_t)(((1ULL << 40) - 1) - (key & ((1ULL << 40) - 1))) : -1;
    }
    return GS_OK;
}

extern "C" int gs_match_max_contig_reads(gs_run *run, int64_t *read_no) {
    if (!run || !read_no) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    const size_t nv = (size_t)run->db->info.n_values;
    std::vector<int64_t> maxk(nv);
    {
        const int frc = fold_stats(run);
        if (frc) return frc;
    }
    HIP_TRY(hipMemcpyAsync(maxk.data(), run->d_max, sizeof(int64_t) * nv, hipMemcpyDeviceToHost, run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    int rc = timer_collect(run->timer);
    if (rc) return rc;
    for (size_t v = 0; v < nv; v++) {
        const u64 key = (u64)maxk[v];
        read_no[v] = key ? (int64_t)(((1ULL << 40) - 1) - (key & ((1ULL << 40) - 1))) : -1;
    }
    return GS_OK;
}

extern "C" int gs_match_reset(gs_run *run) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    if (!run->timer.pending.empty()) HIP_TRY(hipStreamSynchronize(run->stream));
    int rc = timer_collect(run->timer);
    if (rc) return rc;
    rc = run_clear(run);  // kernel-time counters stay cumulative over the life of the handle
    if (rc) return rc;
    return text_reset(run->text, true, run->stream, true);
}

extern "C" int gs_match_destroy(gs_run *run) {
    if (!run) return GS_OK;
    hipSetDevice(run->db->device);
    hipStreamSynchronize(run->stream);
    if (run->db->unique_owner == run) {
        if (run->seen_dirty && !run->db->striped())
            gs_launch_clear_seen(run->db->d_table, run->db->n_slots(), run->db->d_rec, run->db->n_rec, run->stream);
        hipStreamSynchronize(run->stream);
        run->db->unique_owner = nullptr;
    }
    gs_db *db = run->db;
    run_free(run);
    if (--db->live_runs == 0 && db->destroy_pending) db_free(db);
    return GS_OK;
}

extern "C" int gs_match_device_state(gs_run *run, void **sums, void **max_keys, void **dsums, void **bitmap,
                                     int64_t *bitmap_words) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    {
        const int frc = fold_stats(run);
        if (frc) return frc;
    }
    if (bitmap && run->cfg.count_unique && !run->bitmap_merged) {  // refresh the compact copy of the seen bits
        const int xrc = run_extract_bitmap(run);
        if (xrc) return xrc;
    }
    HIP_TRY(hipStreamSynchronize(run->stream));
    if (sums) *sums = run->d_sums;
    if (max_keys) *max_keys = run->d_max;
    if (dsums) *dsums = run->d_dsums;
    if (bitmap) *bitmap = run->d_bitmap;
    if (bitmap_words) *bitmap_words = run->bitmap_words;
    return GS_OK;
}

extern "C" int gs_match_or_bitmap(gs_run *run, const void *parts, int64_t n_parts) {
    if (!run || !parts || n_parts < 1) return fail(GS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(run->db->device));
    {
        const int src = bitmap_settle(run);
        if (src) return src;
    }
    HIP_TRY(gs_launch_bitmap_or(run->d_bitmap, (const uint32_t *)parts, run->bitmap_words, n_parts, run->stream));
    run->bitmap_written = true;
    HIP_TRY(hipStreamSynchronize(run->stream));
    run->bitmap_merged = true;  // gs_match_finish counts from this merged bitmap
    return GS_OK;
}

// ---- merge of runs that live in one process (gs_merge.hip)
extern "C" int gs_match_merge(gs_run *const *runs, int n_runs) try {
    if (!runs || n_runs < 1) return fail(GS_E_INVALID, "bad argument");
    for (int i = 0; i < n_runs; i++) {
        if (!runs[i]) return fail(GS_E_INVALID, "run is NULL");
        for (int j = 0; j < i; j++)
            if (runs[j] == runs[i]) return fail(GS_E_INVALID, "the same run twice");
    }
    const gs_run *r0 = runs[0];
    const gs_db_info &i0 = r0->db->info;
    for (int i = 1; i < n_runs; i++) {  // the stores must be replicas: the bitmap is indexed by table slot / record offset
        const gs_db_info &x = runs[i]->db->info;
        if (x.k != i0.k || x.n_values != i0.n_values || x.n_stored != i0.n_stored || x.n_buckets != i0.n_buckets ||
            x.rec_bytes != i0.rec_bytes || x.n_in_records != i0.n_in_records || runs[i]->bitmap_words != r0->bitmap_words)
            return fail(GS_E_INVALID, "gs_match_merge needs runs on replicas of one store");
        if (runs[i]->cfg.count_unique != r0->cfg.count_unique) return fail(GS_E_INVALID, "runs differ in count_unique");
        if ((runs[i]->d_hit_counts != nullptr) != (r0->d_hit_counts != nullptr)) return fail(GS_E_INVALID, "runs differ in max_kmer_res_counts");
    }
    const size_t nv = (size_t)i0.n_values;
    const bool uniq = r0->cfg.count_unique != 0;
    const int64_t words = r0->bitmap_words;
    // every run's compact bitmap up to date, every stream drained
    for (int i = 0; i < n_runs; i++) {
        gs_run *run = runs[i];
        HIP_TRY(hipSetDevice(run->db->device));
        {
            const int frc = fold_stats(run);
            if (frc) return frc;
        }
        if (uniq && !run->bitmap_merged) {
            const int xrc = run_extract_bitmap(run);
            if (xrc) return xrc;
        }
        HIP_TRY(hipStreamSynchronize(run->stream));
    }
    // per-k-mer hit counters (max_kmer_res_counts > 0, gs_match_max_counts): summed over all runs on the host and written back to
    // every run (uint32 per slot, like the counters themselves; the Java-short wrap happens when they are read)
    if (r0->d_hit_counts) {
        const size_t n_hc = (size_t)(r0->db->n_slots() + r0->db->n_rec * GS_REC_SLOTS);
        std::vector<uint32_t> total(n_hc, 0), part(n_hc);
        for (int i = 0; i < n_runs; i++) {
            HIP_TRY(hipSetDevice(runs[i]->db->device));
            HIP_TRY(hipMemcpy(part.data(), runs[i]->d_hit_counts, n_hc * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t j = 0; j < n_hc; j++) total[j] += part[j];
        }
        for (int i = 0; i < n_runs; i++) {
            HIP_TRY(hipSetDevice(runs[i]->db->device));
            HIP_TRY(hipMemcpy(runs[i]->d_hit_counts, total.data(), n_hc * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    // ---- stage A: the runs of one device into that device's first run (its leader)
    std::vector<int> devices;
    std::vector<gs_run *> leader;
    for (int i = 0; i < n_runs; i++) {
        gs_run *run = runs[i];
        size_t d = 0;
        while (d < devices.size() && devices[d] != run->db->device) d++;
        if (d == devices.size()) {
            devices.push_back(run->db->device);
            leader.push_back(run);
            continue;
        }
        gs_run *L = leader[d];
        HIP_TRY(hipSetDevice(L->db->device));
        HIP_TRY(gs_launch_merge_i64(L->d_sums, run->d_sums, (int64_t)(nv * GS_N_SUMS), 0, L->stream));
        HIP_TRY(gs_launch_merge_i64(L->d_max, run->d_max, (int64_t)nv, 1, L->stream));
        HIP_TRY(gs_launch_merge_f64(L->d_dsums, run->d_dsums, (int64_t)(nv * GS_N_DCOLS), L->stream));
        if (uniq) HIP_TRY(gs_launch_bitmap_or(L->d_bitmap, run->d_bitmap, words, 1, L->stream));
    }
    // ---- stage B: the leaders among each other over RCCL (GS_MERGE_FORCE_RCCL=1: also for a single device, as a rehearsal)
    const int n_dev = (int)devices.size();
    const char *force = getenv("GS_MERGE_FORCE_RCCL");
    if (n_dev > 1 || (force && atoi(force) != 0)) {
        std::vector<void *> ps((size_t)n_dev), pm((size_t)n_dev), pd((size_t)n_dev), pb((size_t)n_dev), pg((size_t)n_dev, nullptr);
        std::vector<hipStream_t> st((size_t)n_dev);
        int rc = GS_OK;
        for (int d = 0; d < n_dev && rc == GS_OK; d++) {
            gs_run *L = leader[(size_t)d];
            ps[(size_t)d] = L->d_sums;
            pm[(size_t)d] = L->d_max;
            pd[(size_t)d] = L->d_dsums;
            pb[(size_t)d] = L->d_bitmap;
            st[(size_t)d] = L->stream;
            if (uniq) {
                hipSetDevice(L->db->device);
                if (gs_dev_alloc(&pg[(size_t)d], sizeof(uint32_t) * (size_t)words * (size_t)n_dev) != hipSuccess)
                    rc = fail(GS_E_NOMEM, "merge scratch");
            }
        }
        const char *msg = "";
        if (rc == GS_OK) {
            const int m = gs_rccl_merge_leaders(n_dev, devices.data(), ps.data(), pm.data(), pd.data(), pb.data(), pg.data(),
                                                (int64_t)(nv * GS_N_SUMS), (int64_t)nv, (int64_t)(nv * GS_N_DCOLS), uniq ? words : 0,
                                                st.data(), &msg);
            if (m != 0) rc = fail(m == -4 ? GS_E_UNSUPPORTED : GS_E_HIP, msg);
        }
        for (int d = 0; d < n_dev && rc == GS_OK; d++) {
            gs_run *L = leader[(size_t)d];
            hipSetDevice(L->db->device);
            if (uniq && gs_launch_bitmap_or(L->d_bitmap, (const uint32_t *)pg[(size_t)d], words, n_dev, L->stream) != hipSuccess)
                rc = fail(GS_E_HIP, "bitmap OR");
            if (rc == GS_OK && hipStreamSynchronize(L->stream) != hipSuccess) rc = fail(GS_E_HIP, "merge sync");
        }
        for (int d = 0; d < n_dev; d++)
            if (pg[(size_t)d]) {
                hipSetDevice(devices[(size_t)d]);
                gs_dev_free(pg[(size_t)d]);
            }
        if (rc != GS_OK) return rc;
    }
    // ---- stage C: the global state back into every run of the device
    for (int i = 0; i < n_runs; i++) {
        gs_run *run = runs[i];
        size_t d = 0;
        while (devices[d] != run->db->device) d++;
        gs_run *L = leader[d];
        HIP_TRY(hipSetDevice(L->db->device));
        if (run != L) {
            HIP_TRY(hipMemcpyAsync(run->d_sums, L->d_sums, sizeof(int64_t) * nv * GS_N_SUMS, hipMemcpyDeviceToDevice, L->stream));
            HIP_TRY(hipMemcpyAsync(run->d_max, L->d_max, sizeof(int64_t) * nv, hipMemcpyDeviceToDevice, L->stream));
            HIP_TRY(hipMemcpyAsync(run->d_dsums, L->d_dsums, sizeof(double) * nv * GS_N_DCOLS, hipMemcpyDeviceToDevice, L->stream));
            if (uniq) HIP_TRY(hipMemcpyAsync(run->d_bitmap, L->d_bitmap, sizeof(uint32_t) * (size_t)words, hipMemcpyDeviceToDevice, L->stream));
        }
        run->bitmap_merged = uniq;  // gs_match_finish counts from the merged bitmap
        run->bitmap_written = run->bitmap_written || uniq;
    }
    for (gs_run *L : leader) {
        HIP_TRY(hipSetDevice(L->db->device));
        HIP_TRY(hipStreamSynchronize(L->stream));
    }
    return GS_OK;
}
GS_API_CATCH


// ---------------------------------------------------------------------------------------------------
// DB construction on the device (gs_build.hip; include/gsgpu.h "gs_dbbuild")
// ---------------------------------------------------------------------------------------------------
// depth of every value index by parent walks (-1: no node); exactly one root: TaxTree.getLowestCommonAncestor answers null for
// nodes of different trees and the update then keeps the old value (DBGoal.java:243), which depends on the order of the regions
static int build_tree_depths(int32_t n_values, const int32_t *parent_vi, std::vector<int32_t> &depth, const char *who) {
    depth.assign((size_t)n_values, -1);
    int roots = 0;
    for (int32_t v = 0; v < n_values; v++) {
        const int32_t p = parent_vi[v];
        if (p < -2 || p >= n_values || p == v) return fail(GS_E_INVALID, "parent_vi out of range");
        roots += p == -1;
    }
    if (roots != 1) return fail(GS_E_UNSUPPORTED, std::string(who) + " needs a tree with exactly one root");
    for (int32_t v = 0; v < n_values; v++) {
        if (parent_vi[v] == -2 || depth[(size_t)v] >= 0) continue;
        std::vector<int32_t> path;
        int32_t x = v;
        while (x >= 0 && depth[(size_t)x] < 0) {
            if (parent_vi[x] == -2) return fail(GS_E_INVALID, "parent_vi points at a value without a node");
            path.push_back(x);
            if ((int32_t)path.size() > n_values) return fail(GS_E_INVALID, "parent_vi contains a cycle");
            x = parent_vi[x];
        }
        int32_t d = x >= 0 ? depth[(size_t)x] + 1 : 0;
        for (size_t i = path.size(); i-- > 0;) depth[(size_t)path[i]] = d++;
    }
    return GS_OK;
}

// ---- The region stage: what gs_dbbuild, gs_dbquality and gs_dbupdate share in front of the builder's k-mer kernel.  All three
// take batches of regions (seq, offsets, one tag per region, mem) under the same parameters and turn them into (k-mer, region)
// pairs with gs_launch_build_kmers; their handles are a RegionStage plus what they do with the pairs.
struct RegionStage {
    int device = 0, k = 0, lower = 1, step = 1, max_dust = -1;
    int32_t n_values = 0;
    hipStream_t stream = nullptr;
    std::vector<int32_t> parent;  // the tree (host copy)
    int32_t *d_tree = nullptr;    // parent | depth, for the handles that fold on the device
    uint8_t *d_seq = nullptr;     // staging of host input
    size_t seq_cap = 0;
    u64 *d_off = nullptr;
    size_t off_cap = 0;
};

// the two parameters every begin takes from its caller; nothing here touches a device
static int region_scan_check(int max_dust, int step_size) {
    if (step_size < 1) return fail(GS_E_INVALID, "stepSize must be >= 1 (C/GSConfigKey.java:236)");
    if (max_dust > 32767) return fail(GS_E_INVALID, "maxDust > Short.MAX_VALUE (C/util/CGATLongBuffer.java:78-80)");
    return GS_OK;
}

// ... and all of them, with the tree's depths, for the begins that fold towards the common ancestor
static int region_params_check(int k, int32_t n_values, const int32_t *parent_vi, int max_dust, int step_size, std::vector<int32_t> &depth,
                               const char *who) {
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (n_values < 1 || n_values > (1 << 24) || !parent_vi) return fail(GS_E_INVALID, "bad tree arrays (n_values must be in [1, 2^24])");
    const int rc = region_scan_check(max_dust, step_size);
    return rc ? rc : build_tree_depths(n_values, parent_vi, depth, who);
}

// parameters and stream on the current device; with depth the tree goes to the device.  A stage that fails here is still freed
// by region_stage_free.
static int region_stage_open(RegionStage *s, int device, int k, int32_t n_values, const int32_t *parent_vi, const int32_t *depth, int lower,
                             int max_dust, int step, const char *who) {
    s->device = device;
    s->k = k;
    s->lower = lower != 0;
    s->step = step;
    s->max_dust = max_dust < 0 ? -1 : max_dust;
    s->n_values = n_values;
    if (parent_vi) s->parent.assign(parent_vi, parent_vi + n_values);  // (gs_dbsize takes no tree)
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess && depth) e = gs_dev_alloc((void **)&s->d_tree, sizeof(int32_t) * 2 * (size_t)n_values);
    if (e == hipSuccess && depth) e = hipMemcpy(s->d_tree, parent_vi, sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice);
    if (e == hipSuccess && depth) e = hipMemcpy(s->d_tree + n_values, depth, sizeof(int32_t) * (size_t)n_values, hipMemcpyHostToDevice);
    return e == hipSuccess ? GS_OK : hip_fail(e, std::string(who) + "_begin");
}

static void region_stage_drop_staging(RegionStage *s) {
    gs_dev_free(s->d_seq);
    gs_dev_free(s->d_off);
    s->d_seq = nullptr;
    s->d_off = nullptr;
    s->seq_cap = s->off_cap = 0;
}

// the end of a handle: waits for the stream, frees the handle's own device buffers (more) and the stage's
static void region_stage_free(RegionStage *s, std::initializer_list<void *> more) {
    hipSetDevice(s->device);
    if (s->stream) hipStreamSynchronize(s->stream);
    for (void *p : more) gs_dev_free(p);
    gs_dev_free(s->d_tree);
    region_stage_drop_staging(s);
    if (s->stream) hipStreamDestroy(s->stream);
}

// a store must be whole on its device to be walked in k-mer order; -> its tree's parents (host)
static int db_whole_store_tree(gs_db *db, const char *who, std::vector<int32_t> &parent) {
    if (db->striped()) return fail(GS_E_UNSUPPORTED, std::string(who) + " needs the whole store on one device: this handle is a stripe");
    HIP_TRY(hipSetDevice(db->device));
    parent.resize((size_t)db->info.n_values);
    HIP_TRY(hipMemcpy(parent.data(), db->d_tree, sizeof(int32_t) * parent.size(), hipMemcpyDeviceToHost));
    return GS_OK;
}

// the offsets of a batch as the host sees them (hoff: the copy of a device batch): from 0, never decreasing -> the batch's bases.
// Every _add checks mem, then its tags, then this.
static int region_batch_check(const uint64_t *offsets, int64_t n_regions, int mem, std::vector<uint64_t> &hoff, int64_t *total) {
    const uint64_t *off = offsets;
    if (mem == GS_MEM_DEVICE) {
        hoff.resize((size_t)n_regions + 1);
        HIP_TRY(hipMemcpy(hoff.data(), offsets, sizeof(uint64_t) * ((size_t)n_regions + 1), hipMemcpyDeviceToHost));
        off = hoff.data();
    }
    if (off[0] != 0) return fail(GS_E_INVALID, "offsets[0] must be 0");
    for (int64_t r = 0; r < n_regions; r++)
        if (off[r + 1] < off[r]) return fail(GS_E_INVALID, "offsets must not decrease");
    *total = (int64_t)off[n_regions];
    return GS_OK;
}

// node_vi is a host array in both cases (one entry per region)
static int region_nodes_check(const RegionStage *s, const int32_t *node_vi, int64_t n_regions) {
    for (int64_t r = 0; r < n_regions; r++)
        if (node_vi[r] < 0 || node_vi[r] >= s->n_values || s->parent[(size_t)node_vi[r]] == -2) return fail(GS_E_INVALID, "node_vi: not a node of the tree");
    return GS_OK;
}

// a whole batch on the device: a host batch through the staging buffers, a device batch where it is
static int region_stage_upload(RegionStage *s, const uint8_t *seq, const uint64_t *offsets, int64_t n_regions, int64_t total, int mem,
                               const uint8_t **d_seq, const u64 **d_off) {
    *d_seq = seq;
    *d_off = (const u64 *)offsets;
    if (mem != GS_MEM_HOST) return GS_OK;
    int rc = grow(&s->d_seq, &s->seq_cap, (size_t)std::max<int64_t>(total, 1), s->stream);
    if (!rc) rc = grow(&s->d_off, &s->off_cap, (size_t)n_regions + 1, s->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_seq, seq, (size_t)total, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_off, offsets, sizeof(u64) * ((size_t)n_regions + 1), hipMemcpyHostToDevice, s->stream));
    *d_seq = s->d_seq;
    *d_off = s->d_off;
    return GS_OK;
}

struct PairBuffer {  // the (k-mer, region | update bit) pairs handed in so far
    u64 *keys = nullptr;
    uint32_t *vals = nullptr;
    size_t cap = 0, n = 0;
    u64 *d_count = nullptr;  // n as the k-mer kernel counts it
};

static int pairs_open(PairBuffer *p, const char *who) {
    hipError_t e = gs_dev_alloc((void **)&p->d_count, sizeof(u64));
    if (e == hipSuccess) e = hipMemset(p->d_count, 0, sizeof(u64));
    return e == hipSuccess ? GS_OK : hip_fail(e, std::string(who) + "_begin");
}

static void pairs_drop(PairBuffer *p) {
    gs_dev_free(p->keys);
    gs_dev_free(p->vals);
    p->keys = nullptr;
    p->vals = nullptr;
    p->cap = p->n = 0;
}

// room for `extra` more pairs: the pair buffers grow by doubling
static int pairs_reserve(PairBuffer *p, size_t extra, hipStream_t stream, const char *who) {
    if (p->n + extra <= p->cap) return GS_OK;
    const size_t want = std::max<size_t>(std::max(p->cap * 2, p->n + extra), 1 << 20);
    u64 *nk = nullptr;
    uint32_t *nv = nullptr;
    hipError_t e = gs_dev_alloc((void **)&nk, want * sizeof(u64));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&nv, want * sizeof(uint32_t));
    if (e == hipSuccess && p->n) e = hipMemcpyAsync(nk, p->keys, p->n * sizeof(u64), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && p->n) e = hipMemcpyAsync(nv, p->vals, p->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        gs_dev_free(nk);
        gs_dev_free(nv);
        return hip_fail(e, who);
    }
    gs_dev_free(p->keys);
    gs_dev_free(p->vals);
    p->keys = nk;
    p->vals = nv;
    p->cap = want;
    return GS_OK;
}

// the k-mers of a batch on the device behind the pairs so far (room for `total` more is reserved); regions count from first_region
static int pairs_append(RegionStage *s, PairBuffer *p, const uint8_t *d_seq, const u64 *d_off, int64_t n_regions, int64_t total,
                        uint32_t first_region, int update, u64 range_lo, u64 range_hi, const char *who) {
    HIP_TRY(gs_launch_build_kmers(d_seq, d_off, n_regions, total, s->k, s->lower, s->step, s->max_dust, first_region, update, range_lo, range_hi,
                                  p->keys, p->vals, p->d_count, s->stream));
    u64 have = 0;
    HIP_TRY(hipMemcpyAsync(&have, p->d_count, sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (the caller's arrays and the staging buffers are free again)
    if (have < p->n || have > p->cap) return fail(GS_E_HIP, std::string(who) + ": pair counter out of range");
    p->n = (size_t)have;
    return GS_OK;
}

// finished arrays (ascending k-mers, their values) on the device: to the host ...
static int sorted_store_fetch(int device, int64_t n, const void *d_keys, const void *d_vals, int64_t *kmers, int32_t *value_idx) {
    HIP_TRY(hipSetDevice(device));
    if (n > 0) {
        HIP_TRY(hipMemcpy(kmers, d_keys, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(value_idx, d_vals, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return GS_OK;
}

// ... or into a store laid out on the device
static int sorted_store_to_db(int device, int k, int32_t n_values, const std::vector<int32_t> &parent_vi, int64_t n, const void *d_keys,
                              const int32_t *d_vals, const char *who, gs_db **out) {
    if (n <= 0 || k < GS_MIN_K || n_values > GS_REC_MAX_VALUES || n >= ((int64_t)1 << 31))
        return fail(GS_E_UNSUPPORTED, std::string(who) + " serves stores with records (k >= 19, at most 2^21 values, 1 .. 2^31 - 1 k-mers): fetch the arrays and call gs_db_create");
    HIP_TRY(hipSetDevice(device));
    std::vector<int32_t> parent, depth, tin, tout;
    int rc = tree_arrays(n_values, parent_vi.data(), parent, depth, tin, tout);
    if (rc) return rc;
    BuildTrace trace;
    rc = db_create_on_device(out, device, k, n, (const int64_t *)d_keys, d_vals, n_values, parent, depth, tin, tout, trace, true);
    if (rc == 0) return fail(GS_E_UNSUPPORTED, std::string(who) + ": no k-mer of these arrays fits a record: fetch the arrays and call gs_db_create");
    return rc < 0 ? rc : GS_OK;
}

struct gs_dbbuild : RegionStage {
    PairBuffer pairs;
    u64 range_lo = 0, range_hi = ~0ULL;  // gs_dbbuild_set_range
    std::vector<int32_t> node_of_region;
    int64_t *d_out_keys = nullptr;
    int32_t *d_out_vals = nullptr;
    int64_t n_out = 0, n_kmers_seen = 0;
    bool finished = false;
    bool failed = false;  // gs_dbbuild_finish failed half-way: the pairs are gone, nothing can be fetched (sticky GS_E_STATE)
};

static void dbbuild_free(gs_dbbuild *b) {
    region_stage_free(b, {b->pairs.keys, b->pairs.vals, b->pairs.d_count, b->d_out_keys, b->d_out_vals});
    delete b;
}

extern "C" int gs_dbbuild_begin(gs_dbbuild **out, int device, int k, int32_t n_values, const int32_t *parent_vi, int lower_case_bases,
                                int max_dust, int step_size) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    std::vector<int32_t> depth;
    int rc = region_params_check(k, n_values, parent_vi, max_dust, step_size, depth, "gs_dbbuild");
    if (rc) return rc;
    rc = use_device(device);
    if (rc) return rc;
    gs_dbbuild *b = new gs_dbbuild();
    rc = region_stage_open(b, device, k, n_values, parent_vi, depth.data(), lower_case_bases, max_dust, step_size, "gs_dbbuild");
    if (!rc) rc = pairs_open(&b->pairs, "gs_dbbuild");
    if (rc) {
        dbbuild_free(b);
        return rc;
    }
    *out = b;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbbuild_add(gs_dbbuild *b, const uint8_t *seq, const uint64_t *offsets, const int32_t *node_vi, int64_t n_regions, int mem,
                              int update) try {
    if (!b || n_regions < 0 || (n_regions > 0 && (!seq || !offsets || !node_vi))) return fail(GS_E_INVALID, "bad argument");
    if (b->finished) return fail(GS_E_STATE, "gs_dbbuild_finish has been called");
    if (n_regions == 0) return GS_OK;
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HIP_TRY(hipSetDevice(b->device));
    if (b->node_of_region.size() + (size_t)n_regions >= ((size_t)1 << 31)) return fail(GS_E_UNSUPPORTED, "more than 2^31 regions");
    std::vector<uint64_t> hoff;
    int64_t total = 0;
    const uint8_t *d_seq = nullptr;
    const u64 *d_off = nullptr;
    int rc = region_nodes_check(b, node_vi, n_regions);
    if (!rc) rc = region_batch_check(offsets, n_regions, mem, hoff, &total);
    if (!rc) rc = region_stage_upload(b, seq, offsets, n_regions, total, mem, &d_seq, &d_off);
    if (!rc) rc = pairs_reserve(&b->pairs, (size_t)total, b->stream, "gs_dbbuild_add");
    if (!rc) rc = pairs_append(b, &b->pairs, d_seq, d_off, n_regions, total, (uint32_t)b->node_of_region.size(), update != 0, b->range_lo,
                               b->range_hi, "gs_dbbuild_add");
    if (rc) return rc;
    b->node_of_region.insert(b->node_of_region.end(), node_vi, node_vi + n_regions);
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbbuild_set_range(gs_dbbuild *b, uint64_t lo, uint64_t hi) {
    if (!b || lo >= hi) return fail(GS_E_INVALID, "bad range");
    if (b->pairs.n > 0 || !b->node_of_region.empty()) return fail(GS_E_STATE, "gs_dbbuild_set_range comes before the first gs_dbbuild_add");
    b->range_lo = lo;
    b->range_hi = hi;
    return GS_OK;
}

extern "C" int gs_dbbuild_finish(gs_dbbuild *b, int64_t *n_kmers) try {
    if (!b || !n_kmers) return fail(GS_E_INVALID, "NULL argument");
    if (b->failed) return fail(GS_E_STATE, "this builder's gs_dbbuild_finish failed: its pairs are gone (start over with gs_dbbuild_begin)");
    if (b->finished) {
        *n_kmers = b->n_out;
        return GS_OK;
    }
    *n_kmers = 0;
    HIP_TRY(hipSetDevice(b->device));
    region_stage_drop_staging(b);
    const int64_t n = (int64_t)b->pairs.n;
    u64 *keys_alt = nullptr, *pos = nullptr;
    uint32_t *vals_alt = nullptr, *flag = nullptr;
    int32_t *value = nullptr, *d_nor = nullptr;
    HipSteps check{"gs_dbbuild_finish"};
    if (n > 0) {
        u64 *ks = nullptr;
        uint32_t *vs = nullptr;
        const u64 n_valid = (u64)n;
        bool ok = check(gs_dev_alloc((void **)&keys_alt, (size_t)n * sizeof(u64)), "sort buffers") &&
                  check(gs_dev_alloc((void **)&vals_alt, (size_t)n * sizeof(uint32_t)), "sort buffers") &&
                  check(gs_build_sort(b->pairs.keys, keys_alt, b->pairs.vals, vals_alt, n, 2 * b->k, &ks, &vs, b->stream), "sort");
        b->n_kmers_seen = (int64_t)n_valid;
        if (ok && n_valid > 0) {
            const size_t nr = std::max<size_t>(b->node_of_region.size(), 1);
            ok = check(gs_dev_alloc((void **)&d_nor, nr * sizeof(int32_t)), "regions") &&
                 check(hipMemcpy(d_nor, b->node_of_region.data(), b->node_of_region.size() * sizeof(int32_t), hipMemcpyHostToDevice), "regions") &&
                 check(gs_dev_alloc((void **)&flag, (size_t)n_valid * sizeof(uint32_t)), "scratch") &&
                 check(gs_dev_alloc((void **)&value, (size_t)n_valid * sizeof(int32_t)), "scratch") &&
                 check(gs_dev_alloc((void **)&pos, (size_t)n_valid * sizeof(u64)), "scratch") &&
                 check(gs_build_reduce(ks, vs, (int64_t)n_valid, d_nor, b->d_tree, b->d_tree + b->n_values, flag, value, pos, &b->n_out, b->stream), "reduce");
            if (ok && b->n_out > 0)
                ok = check(gs_dev_alloc((void **)&b->d_out_keys, (size_t)b->n_out * sizeof(int64_t)), "result") &&
                     check(gs_dev_alloc((void **)&b->d_out_vals, (size_t)b->n_out * sizeof(int32_t)), "result") &&
                     check(gs_launch_build_scatter(ks, value, flag, pos, (int64_t)n_valid, b->d_out_keys, b->d_out_vals, b->stream), "scatter") &&
                     check(hipStreamSynchronize(b->stream), "scatter");
        }
    }
    for (void *p : {(void *)keys_alt, (void *)vals_alt, (void *)pos, (void *)flag, (void *)value, (void *)d_nor}) gs_dev_free(p);
    pairs_drop(&b->pairs);
    if (check.rc != GS_OK) {  // nothing half-built may be handed out later: no results, no second finish
        gs_dev_free(b->d_out_keys);
        gs_dev_free(b->d_out_vals);
        b->d_out_keys = nullptr;
        b->d_out_vals = nullptr;
        b->n_out = 0;
        b->failed = true;
        return check.rc;
    }
    b->finished = true;
    *n_kmers = b->n_out;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbbuild_fetch(gs_dbbuild *b, int64_t *kmers, int32_t *value_idx) {
    if (!b || (b->n_out > 0 && (!kmers || !value_idx))) return fail(GS_E_INVALID, "NULL argument");
    if (!b->finished) return fail(GS_E_STATE, "gs_dbbuild_finish first");
    return sorted_store_fetch(b->device, b->n_out, b->d_out_keys, b->d_out_vals, kmers, value_idx);
}

extern "C" int gs_dbbuild_to_db(gs_dbbuild *b, gs_db **out) try {
    if (!b || !out) return fail(GS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (!b->finished) return fail(GS_E_STATE, "gs_dbbuild_finish first");
    return sorted_store_to_db(b->device, b->k, b->n_values, b->parent, b->n_out, b->d_out_keys, b->d_out_vals, "gs_dbbuild_to_db", out);
}
GS_API_CATCH

extern "C" int gs_dbbuild_destroy(gs_dbbuild *b) {
    if (b) dbbuild_free(b);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// Store quality against its source genomes (gs_quality.hip; include/gsgpu.h "gs_dbquality")
// ---------------------------------------------------------------------------------------------------
struct gs_dbquality : RegionStage {  // (parent: the store's tree; no d_tree, the join reads the store's own)
    gs_db *db = nullptr;
    PairBuffer pairs;  // the (k-mer, leaf) pairs of this pass
    u64 range_lo = 0, range_hi = ~0ULL;
    uint32_t *d_leaf = nullptr;  // leaf of each region of one add
    size_t leaf_cap = 0;
    int32_t one_leaf = -1;  // all regions so far carry this tag (-2: several)
    bool added = false, finished = false;
    gs_dbexport *store = nullptr;       // the store in ascending k-mer order, decoded once per handle
    std::vector<int64_t> value_counts;  // gs_db_value_counts, once per handle
    gs_dbquality_stats stats{};
};

static void dbquality_free(gs_dbquality *q) {
    region_stage_free(q, {q->pairs.keys, q->pairs.vals, q->pairs.d_count, q->d_leaf});
    if (q->store) gs_dbexport_destroy(q->store);
    delete q;
}

extern "C" int gs_dbquality_begin(gs_dbquality **out, gs_db *db, int lower_case_bases, int max_dust, int step_size) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!db) return fail(GS_E_INVALID, "db is NULL");
    std::vector<int32_t> parent;
    int rc = region_scan_check(max_dust, step_size);
    if (!rc) rc = db_whole_store_tree(db, "gs_dbquality", parent);
    if (rc) return rc;
    gs_dbquality *q = new gs_dbquality();
    q->db = db;
    rc = region_stage_open(q, db->device, db->info.k, db->info.n_values, parent.data(), nullptr, lower_case_bases, max_dust, step_size, "gs_dbquality");
    if (!rc) rc = pairs_open(&q->pairs, "gs_dbquality");
    if (rc) {
        dbquality_free(q);
        return rc;
    }
    *out = q;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbquality_set_range(gs_dbquality *q, uint64_t lo, uint64_t hi) {
    if (!q || lo >= hi) return fail(GS_E_INVALID, "bad range");
    if (q->added && !q->finished) return fail(GS_E_STATE, "gs_dbquality_set_range comes before the first gs_dbquality_add of a pass");
    q->range_lo = lo;
    q->range_hi = hi;
    q->finished = false;  // (after gs_dbquality_finish: the next pass over the same store)
    q->added = false;
    q->one_leaf = -1;
    q->stats.ms_pairs = 0;
    return GS_OK;
}

extern "C" int gs_dbquality_add(gs_dbquality *q, const uint8_t *seq, const uint64_t *offsets, const int32_t *leaf_vi, int64_t n_regions,
                                int mem) try {
    if (!q || n_regions < 0 || (n_regions > 0 && (!seq || !offsets || !leaf_vi))) return fail(GS_E_INVALID, "bad argument");
    if (q->finished) return fail(GS_E_STATE, "gs_dbquality_finish has been called (gs_dbquality_set_range starts another pass)");
    if (n_regions == 0) return GS_OK;
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (n_regions >= ((int64_t)1 << 31)) return fail(GS_E_UNSUPPORTED, "more than 2^31 regions");
    HIP_TRY(hipSetDevice(q->device));
    // leaf_vi is a host array in both cases; negative or a value without a node: the region counts nothing (leafNode == null)
    std::vector<uint32_t> leaf((size_t)n_regions);
    int32_t one = q->one_leaf;
    for (int64_t r = 0; r < n_regions; r++) {
        const int32_t v = leaf_vi[r];
        if (v >= q->n_values) return fail(GS_E_INVALID, "leaf_vi: not a value of the store");
        const int32_t tag = (v < 0 || q->parent[(size_t)v] == -2) ? q->n_values : v;
        leaf[(size_t)r] = (uint32_t)tag;
        one = one == -1 ? tag : (one == tag ? one : -2);
    }
    std::vector<uint64_t> hoff;
    int64_t total = 0;
    const uint8_t *d_seq = nullptr;
    const u64 *d_off = nullptr;
    int rc = region_batch_check(offsets, n_regions, mem, hoff, &total);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    rc = grow(&q->d_leaf, &q->leaf_cap, (size_t)n_regions, q->stream);
    if (!rc) rc = region_stage_upload(q, seq, offsets, n_regions, total, mem, &d_seq, &d_off);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(q->d_leaf, leaf.data(), sizeof(uint32_t) * (size_t)n_regions, hipMemcpyHostToDevice, q->stream));
    // the builder's kernel with region numbers from 0, then region -> leaf on the pairs it has just written
    const size_t before = q->pairs.n;
    rc = pairs_reserve(&q->pairs, (size_t)total, q->stream, "gs_dbquality_add");
    if (!rc) rc = pairs_append(q, &q->pairs, d_seq, d_off, n_regions, total, 0u, 0, q->range_lo, q->range_hi, "gs_dbquality_add");
    if (rc) return rc;
    HIP_TRY(gs_launch_quality_tag(q->pairs.vals + before, (int64_t)(q->pairs.n - before), q->d_leaf, n_regions, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));  // (d_leaf is free again)
    q->one_leaf = one;
    q->added = true;
    q->stats.ms_pairs += ms_since(t0);
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbquality_finish(gs_dbquality *q, int64_t *counts, uint8_t *present) try {
    if (!q || !counts || !present) return fail(GS_E_INVALID, "NULL argument");
    if (q->finished) return fail(GS_E_STATE, "gs_dbquality_finish has been called (gs_dbquality_set_range starts another pass)");
    HIP_TRY(hipSetDevice(q->device));
    const int32_t nv = q->n_values;
    const int64_t n = (int64_t)q->pairs.n;
    using clk = std::chrono::steady_clock;
    u64 *keys_alt = nullptr, *d_cnt = nullptr;
    uint32_t *vals_alt = nullptr;
    std::vector<u64> h_cnt(2 * (size_t)nv + 2, 0);
    HipSteps check{"gs_dbquality_finish"};
    region_stage_drop_staging(q);  // the staging buffers make room for the sort
    gs_dev_free(q->d_leaf);
    q->d_leaf = nullptr;
    q->leaf_cap = 0;
    q->stats.n_pairs = n;
    q->stats.n_distinct = q->stats.n_found = 0;
    q->stats.ms_sort = q->stats.ms_join = 0;
    // once per handle: the store in ascending k-mer order on the device, and its k-mers per value
    if (!q->store) {
        const auto t0 = clk::now();
        int64_t m = 0;
        int rc = gs_dbexport_create(&q->store, q->db, -1, 0, &m);
        if (rc == GS_OK) {
            q->value_counts.assign((size_t)nv, 0);
            rc = gs_db_value_counts(q->db, q->value_counts.data());
        }
        if (rc != GS_OK) {
            if (q->store) gs_dbexport_destroy(q->store);
            q->store = nullptr;
            return rc;
        }
        HIP_TRY(hipSetDevice(q->device));
        q->stats.ms_decode = ms_since(t0);
        q->stats.n_store = m;
    }
    if (n > 0) {
        u64 *ks = q->pairs.keys;
        uint32_t *vs = q->pairs.vals;
        auto t0 = clk::now();
        bool ok = check(gs_dev_alloc((void **)&keys_alt, (size_t)n * sizeof(u64)), "sort buffers") &&
                  check(gs_dev_alloc((void **)&vals_alt, (size_t)n * sizeof(uint32_t)), "sort buffers");
        if (ok && q->one_leaf == -2) {  // several leaves: the leaf bits first, the stable k-mer sort keeps their order
            int bits = 1;
            while (((int64_t)1 << bits) <= (int64_t)nv) bits++;
            ok = check(gs_quality_sort_leaf(q->pairs.vals, vals_alt, q->pairs.keys, keys_alt, n, bits, &vs, &ks, q->stream), "leaf sort");
        }
        if (ok) {
            u64 *ka = ks == q->pairs.keys ? keys_alt : q->pairs.keys;
            uint32_t *va = vs == q->pairs.vals ? vals_alt : q->pairs.vals;
            ok = check(gs_build_sort(ks, ka, vs, va, n, 2 * q->k, &ks, &vs, q->stream), "sort");
        }
        q->stats.ms_sort = ms_since(t0);
        t0 = clk::now();
        if (ok) {
            GsQualityParams P{};
            P.keys = ks;
            P.leaf = vs;
            P.n = n;
            P.skeys = q->store->d_keys;
            P.svals = q->store->d_vals;
            P.m = q->store->n;
            P.tin = q->db->dev.tin;
            P.tout = q->db->dev.tout;
            P.n_values = nv;
            ok = check(gs_dev_alloc((void **)&d_cnt, h_cnt.size() * sizeof(u64)), "counts") &&
                 check(hipMemsetAsync(d_cnt, 0, h_cnt.size() * sizeof(u64), q->stream), "counts");
            P.counts = d_cnt;
            P.stats = d_cnt + 2 * (size_t)nv;
            ok = ok && check(gs_launch_quality_join(&P, q->db->n_cu, q->stream), "join") &&
                 check(hipMemcpyAsync(h_cnt.data(), d_cnt, h_cnt.size() * sizeof(u64), hipMemcpyDeviceToHost, q->stream), "counts") &&
                 check(hipStreamSynchronize(q->stream), "join");
        }
        q->stats.ms_join = ms_since(t0);
    }
    gs_dev_free(keys_alt);
    gs_dev_free(vals_alt);
    gs_dev_free(d_cnt);
    pairs_drop(&q->pairs);
    HIP_TRY(hipMemset(q->pairs.d_count, 0, sizeof(u64)));
    q->finished = true;  // (also after a failure: the pairs are gone)
    if (check.rc != GS_OK) return check.rc;
    q->stats.n_distinct = (int64_t)h_cnt[2 * (size_t)nv];
    q->stats.n_found = (int64_t)h_cnt[2 * (size_t)nv + 1];
    // tp+fp: the stored k-mers on the path leaf -> root (getPathSum, DBQualityCountsGoal.java:137-147, :315-321)
    for (int32_t v = 0; v < nv; v++) {
        int64_t *row = counts + 3 * (size_t)v;
        row[0] = row[1] = row[2] = 0;
        present[v] = 0;
        if (h_cnt[2 * (size_t)v + 1] == 0) continue;
        present[v] = 1;
        row[0] = (int64_t)h_cnt[2 * (size_t)v];
        row[2] = (int64_t)h_cnt[2 * (size_t)v + 1];
        for (int32_t a = v; a >= 0; a = q->parent[(size_t)a]) row[1] += q->value_counts[(size_t)a];
    }
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbquality_get_stats(gs_dbquality *q, gs_dbquality_stats *out) {
    if (!q || !out) return fail(GS_E_INVALID, "NULL argument");
    *out = q->stats;
    return GS_OK;
}

extern "C" int gs_dbquality_destroy(gs_dbquality *q) {
    if (q) dbquality_free(q);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// A finished store updated in batches (gs_update.hip; include/gsgpu.h "gs_dbupdate")
// ---------------------------------------------------------------------------------------------------
#define GS_UPD_DEFAULT_SLICE ((int64_t)1 << 25)  // bases per slice: 13 bytes of working memory each (436 MB)

struct gs_dbupdate : RegionStage {
    int n_cu = 256;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    // the store: lives as long as the handle
    int64_t n = 0;
    u64 *d_keys = nullptr;       // ascending, never written
    int32_t *d_vals = nullptr;   // updated in place
    int32_t *d_vals0 = nullptr;  // the values at begin (n_moved)
    void *d_dir = nullptr;
    int dir_bits = 1;
    bool wide = false;
    u64 *d_cnt = nullptr;  // [0] pairs of the slice (the k-mer kernel's counter), [1] pairs so far, [2] found so far, [3] moved; then the check flag
    // one slice's working memory (with the stage's d_seq / d_off, which hold a slice here and exactly that: dbupdate_room): sized
    // by the largest slice so far, never by the number of calls
    int64_t slice_bases = GS_UPD_DEFAULT_SLICE;
    int32_t *d_node = nullptr;
    u64 *d_pkeys = nullptr;
    uint32_t *d_pvals = nullptr;
    size_t node_cap = 0, pair_cap = 0;
    bool finished = false;
    bool failed = false;  // a device error in the middle of an add: the values are half-updated (sticky GS_E_STATE)
    int64_t n_moved = 0;
    gs_dbupdate_stats stats{};
};

static void dbupdate_free(gs_dbupdate *u) {
    region_stage_free(u, {u->d_keys, u->d_vals, u->d_vals0, u->d_dir, u->d_cnt, u->d_node, u->d_pkeys, u->d_pvals});
    for (hipEvent_t e : u->ev)
        if (e) hipEventDestroy(e);
    delete u;
}

static int64_t dbupdate_max_regions(const gs_dbupdate *u) { return u->slice_bases / 8 + 64; }

// handle + stream + tree on the current device
static int dbupdate_open(gs_dbupdate **out, int device, int k, int32_t n_values, const int32_t *parent_vi, const std::vector<int32_t> &depth, int lower,
                         int max_dust, int step) {
    gs_dbupdate *u = new gs_dbupdate();
    int rc = region_stage_open(u, device, k, n_values, parent_vi, depth.data(), lower, max_dust, step, "gs_dbupdate");
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) u->n_cu = cu;
    if (!rc) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreate(&u->ev[i]);
        if (e == hipSuccess) e = gs_dev_alloc((void **)&u->d_cnt, 5 * sizeof(u64));
        if (e == hipSuccess) e = hipMemsetAsync(u->d_cnt, 0, 5 * sizeof(u64), u->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(u->stream);
        if (e != hipSuccess) rc = hip_fail(e, "gs_dbupdate_begin");
    }
    if (rc) {
        dbupdate_free(u);
        return rc;
    }
    *out = u;
    return GS_OK;
}

// u->d_keys / u->d_vals / u->n are set: one pass checks them, then the copy of the values and the directory
static int dbupdate_adopt(gs_dbupdate *u, bool check) {
    const int64_t n = u->n;
    if (check && n > 0) {
        uint32_t flag = 0;
        HIP_TRY(hipMemsetAsync(u->d_cnt + 4, 0, sizeof(u64), u->stream));
        HIP_TRY(gs_launch_update_check(u->d_keys, u->d_vals, n, u->k, u->n_values, (uint32_t *)(u->d_cnt + 4), u->n_cu, u->stream));
        HIP_TRY(hipMemcpyAsync(&flag, u->d_cnt + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, u->stream));
        HIP_TRY(hipStreamSynchronize(u->stream));
        if (flag & 1u) return fail(GS_E_INVALID, "kmers must be ascending, distinct and below 4^k");
        if (flag & 2u) return fail(GS_E_INVALID, "value_idx out of range");
    }
    // about two to four k-mers per bucket, never more buckets than 4^k
    int bits = 1;
    while (bits < 31 && bits < 2 * u->k && ((int64_t)2 << bits) <= n) bits++;
    u->dir_bits = bits;
    u->wide = n >= ((int64_t)1 << 32);
    const size_t dir_bytes = (((size_t)1 << bits) + 1) * (u->wide ? 8 : 4);
    HIP_TRY(gs_dev_alloc((void **)&u->d_vals0, std::max<size_t>((size_t)n, 1) * sizeof(int32_t)));
    HIP_TRY(gs_dev_alloc(&u->d_dir, dir_bytes));
    if (n > 0) HIP_TRY(hipMemcpyAsync(u->d_vals0, u->d_vals, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, u->stream));
    HIP_TRY(gs_launch_update_dir(u->d_keys, n, u->k, bits, u->wide ? 1 : 0, u->d_dir, u->n_cu, u->stream));
    HIP_TRY(hipStreamSynchronize(u->stream));
    u->stats.n_store = n;
    u->stats.store_bytes = (int64_t)((size_t)n * (sizeof(u64) + 2 * sizeof(int32_t)) + dir_bytes + sizeof(int32_t) * 2 * (size_t)u->n_values);
    return GS_OK;
}

// the store's arrays copied into the handle (n_kmers pairs from either memory), then dbupdate_adopt; the handle goes on failure
static int dbupdate_copy_in(gs_dbupdate *u, const void *kmers, const void *value_idx, int64_t n_kmers, hipMemcpyKind kind, bool check,
                            const char *who) {
    u->n = n_kmers;
    const size_t m = std::max<size_t>((size_t)n_kmers, 1);
    hipError_t e = gs_dev_alloc((void **)&u->d_keys, m * sizeof(u64));
    if (e == hipSuccess) e = gs_dev_alloc((void **)&u->d_vals, m * sizeof(int32_t));
    // (on the handle's stream: a device-to-device hipMemcpy need not be complete when it returns, and this stream does not wait for the null stream)
    if (e == hipSuccess && n_kmers > 0) e = hipMemcpyAsync(u->d_keys, kmers, (size_t)n_kmers * sizeof(u64), kind, u->stream);
    if (e == hipSuccess && n_kmers > 0) e = hipMemcpyAsync(u->d_vals, value_idx, (size_t)n_kmers * sizeof(int32_t), kind, u->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(u->stream);  // (the caller's arrays are free again)
    const int rc = e != hipSuccess ? hip_fail(e, who) : dbupdate_adopt(u, check);
    if (rc) dbupdate_free(u);
    return rc;
}

extern "C" int gs_dbupdate_begin(gs_dbupdate **out, int device, int k, int32_t n_values, const int32_t *parent_vi, int lower_case_bases,
                                 int max_dust, int step_size, const int64_t *kmers, const int32_t *value_idx, int64_t n_kmers, int mem) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_kmers < 0 || (n_kmers > 0 && (!kmers || !value_idx))) return fail(GS_E_INVALID, "bad store arrays");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    std::vector<int32_t> depth;
    int rc = region_params_check(k, n_values, parent_vi, max_dust, step_size, depth, "gs_dbupdate");
    if (rc) return rc;
    rc = use_device(device);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    gs_dbupdate *u = nullptr;
    rc = dbupdate_open(&u, device, k, n_values, parent_vi, depth, lower_case_bases, max_dust, step_size);
    if (!rc) rc = dbupdate_copy_in(u, kmers, value_idx, n_kmers, mem == GS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, true, "gs_dbupdate_begin");
    if (rc) return rc;
    u->stats.ms_begin = ms_since(t0);
    *out = u;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbupdate_begin_db(gs_dbupdate **out, gs_db *db, int lower_case_bases, int max_dust, int step_size) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!db) return fail(GS_E_INVALID, "db is NULL");
    std::vector<int32_t> parent, depth;
    int rc = region_scan_check(max_dust, step_size);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t nv = db->info.n_values;
    rc = db_whole_store_tree(db, "gs_dbupdate", parent);
    if (!rc) rc = region_params_check(db->info.k, nv, parent.data(), max_dust, step_size, depth, "gs_dbupdate");
    if (rc) return rc;
    // the store in ascending k-mer order, decoded on the device (seen bits masked); its arrays move into the handle
    gs_dbexport *x = nullptr;
    int64_t m = 0;
    rc = gs_dbexport_create(&x, db, -1, 0, &m);
    if (rc) return rc;
    gs_dbupdate *u = nullptr;
    rc = dbupdate_open(&u, db->device, db->info.k, nv, parent.data(), depth, lower_case_bases, max_dust, step_size);
    if (rc) {
        gs_dbexport_destroy(x);
        return rc;
    }
    u->n_cu = db->n_cu;
    u->n = m;
    u->d_keys = x->d_keys;
    u->d_vals = (int32_t *)x->d_vals;
    x->d_keys = nullptr;
    x->d_vals = nullptr;
    gs_dbexport_destroy(x);
    rc = dbupdate_adopt(u, false);  // (the decode emits values below n_values only, and the sort made the order)
    if (rc) {
        dbupdate_free(u);
        return rc;
    }
    u->stats.ms_begin = ms_since(t0);
    *out = u;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbupdate_begin_build(gs_dbupdate **out, gs_dbbuild *b) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!b) return fail(GS_E_INVALID, "builder is NULL");
    if (!b->finished) return fail(GS_E_STATE, "gs_dbbuild_finish first");
    HIP_TRY(hipSetDevice(b->device));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> depth;
    int rc = region_params_check(b->k, b->n_values, b->parent.data(), b->max_dust, b->step, depth, "gs_dbupdate");
    if (rc) return rc;
    gs_dbupdate *u = nullptr;
    rc = dbupdate_open(&u, b->device, b->k, b->n_values, b->parent.data(), depth, b->lower, b->max_dust, b->step);
    // device-to-device: the builder keeps its own arrays for gs_dbbuild_fetch / _to_db
    if (!rc) rc = dbupdate_copy_in(u, b->d_out_keys, b->d_out_vals, b->n_out, hipMemcpyDeviceToDevice, false, "gs_dbupdate_begin_build");
    if (rc) return rc;
    u->stats.ms_begin = ms_since(t0);
    *out = u;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbupdate_set_slice(gs_dbupdate *u, int64_t max_bases) {
    if (!u) return fail(GS_E_INVALID, "NULL argument");
    // a cut region goes on (k - 1) bases earlier and whole steps later: a slice must hold k - 1 + step_size bases
    if (max_bases < (int64_t)u->k - 1 + u->step) return fail(GS_E_INVALID, "a slice holds at least k - 1 + step_size bases");
    if (max_bases > ((int64_t)1 << 31)) return fail(GS_E_INVALID, "a slice holds at most 2^31 bases");
    u->slice_bases = max_bases;
    return GS_OK;
}

// exactly `need`, no slack (grow adds a quarter): batch_bytes_peak is a reported figure
template <typename T>
static hipError_t dbupdate_room(T **p, size_t *cap, size_t need) {
    if (*cap >= need) return hipSuccess;
    gs_dev_free(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = gs_dev_alloc((void **)p, need * sizeof(T));
    if (e == hipSuccess) *cap = need;
    return e;
}

extern "C" int gs_dbupdate_add(gs_dbupdate *u, const uint8_t *seq, const uint64_t *offsets, const int32_t *node_vi, int64_t n_regions,
                               int mem) try {
    if (!u || n_regions < 0 || (n_regions > 0 && (!seq || !offsets || !node_vi))) return fail(GS_E_INVALID, "bad argument");
    if (u->failed) return fail(GS_E_STATE, "an earlier gs_dbupdate_add failed on the device: the values are half-updated (start over)");
    if (u->finished) return fail(GS_E_STATE, "gs_dbupdate_finish has been called");
    if (n_regions == 0) return GS_OK;
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HIP_TRY(hipSetDevice(u->device));
    std::vector<uint64_t> hoff;
    int64_t total = 0;
    int rc = region_nodes_check(u, node_vi, n_regions);
    if (!rc) rc = region_batch_check(offsets, n_regions, mem, hoff, &total);
    if (rc) return rc;
    const uint64_t *off = mem == GS_MEM_DEVICE ? hoff.data() : offsets;
    const int64_t slice = u->slice_bases, max_regions = dbupdate_max_regions(u);
    // all of the call's working memory before any of its work: an out-of-memory leaves the values as they were
    {
        const size_t bases = (size_t)std::max<int64_t>(std::min(slice, total), 1), regions = (size_t)std::min(max_regions, n_regions);
        HIP_TRY(hipStreamSynchronize(u->stream));
        hipError_t e = mem == GS_MEM_HOST ? dbupdate_room(&u->d_seq, &u->seq_cap, bases) : hipSuccess;
        if (e == hipSuccess) e = dbupdate_room(&u->d_off, &u->off_cap, regions + 1);
        if (e == hipSuccess) e = dbupdate_room(&u->d_node, &u->node_cap, regions);
        if (e == hipSuccess) {  // (both pair arrays under one capacity)
            size_t c1 = u->pair_cap, c2 = u->pair_cap;
            e = dbupdate_room(&u->d_pkeys, &c1, bases);
            if (e == hipSuccess) e = dbupdate_room(&u->d_pvals, &c2, bases);
            u->pair_cap = std::min(c1, c2);
        }
        if (e != hipSuccess) return hip_fail(e, "gs_dbupdate_add");
        const int64_t bytes = (int64_t)(u->seq_cap + u->off_cap * sizeof(u64) + u->node_cap * sizeof(int32_t) + u->pair_cap * (sizeof(u64) + sizeof(uint32_t)));
        u->stats.batch_bytes_peak = std::max(u->stats.batch_bytes_peak, bytes);
    }
    GsUpdateParams P{};
    P.skeys = u->d_keys;
    P.svals = u->d_vals;
    P.m = u->n;
    P.dir = u->d_dir;
    P.dir_bits = u->dir_bits;
    P.wide = u->wide ? 1 : 0;
    P.k = u->k;
    P.parent = u->d_tree;
    P.depth = u->d_tree + u->n_values;
    P.keys = u->d_pkeys;
    P.region = u->d_pvals;
    P.n_pairs = u->d_cnt;
    P.node_of_region = u->d_node;
    P.stats = u->d_cnt + 1;
    // Slices: consecutive bytes [begin, begin + used) of the batch, cut into the pieces of regions they hold.  A region that
    // does not fit is cut at a multiple of step_size behind its start (so that (bases of the region so far) % step_size is the
    // same in the piece) and the slice ends there; the next piece starts k - 1 bases before the cut's end: every window lies
    // in exactly one piece.
    std::vector<uint64_t> soff;
    std::vector<int32_t> snode;
    HipSteps check{"gs_dbupdate_add"};
    int64_t r = 0, c = 0;  // the next piece starts c bases into region r
    while (r < n_regions && check.rc == GS_OK) {
        soff.assign(1, 0);
        snode.clear();
        const int64_t begin = (int64_t)off[r] + c;
        int64_t used = 0;
        while (r < n_regions && (int64_t)snode.size() < max_regions) {
            const int64_t rem = (int64_t)(off[r + 1] - off[r]) - c, room = slice - used;
            if (rem <= room) {
                used += rem;
                soff.push_back((uint64_t)used);
                snode.push_back(node_vi[r]);
                r++;
                c = 0;
                continue;
            }
            const int64_t adv = room >= u->k - 1 + u->step ? (room - (u->k - 1)) / u->step * u->step : 0;
            if (adv > 0) {
                used += adv + u->k - 1;
                soff.push_back((uint64_t)used);
                snode.push_back(node_vi[r]);
                c += adv;
            }
            break;
        }
        if (used == 0) continue;  // (empty regions only)
        const int64_t n_sl = (int64_t)snode.size();
        const uint8_t *d_seq = seq + begin;
        if (mem == GS_MEM_HOST) {
            check(hipMemcpyAsync(u->d_seq, seq + begin, (size_t)used, hipMemcpyHostToDevice, u->stream), "copy");
            d_seq = u->d_seq;
        }
        bool ok = check.rc == GS_OK && check(hipMemcpyAsync(u->d_off, soff.data(), sizeof(u64) * ((size_t)n_sl + 1), hipMemcpyHostToDevice, u->stream), "copy") &&
                  check(hipMemcpyAsync(u->d_node, snode.data(), sizeof(int32_t) * (size_t)n_sl, hipMemcpyHostToDevice, u->stream), "copy") &&
                  check(hipMemsetAsync(u->d_cnt, 0, sizeof(u64), u->stream), "counter") && check(hipEventRecord(u->ev[0], u->stream), "event") &&
                  check(gs_launch_build_kmers(d_seq, u->d_off, n_sl, used, u->k, u->lower, u->step, u->max_dust, 0u, 0, 0, ~0ULL, u->d_pkeys, u->d_pvals,
                                              u->d_cnt, u->stream), "k-mers") &&
                  check(hipEventRecord(u->ev[1], u->stream), "event") && check(gs_launch_update_lookup(&P, used, u->n_cu, u->stream), "lookup") &&
                  check(hipEventRecord(u->ev[2], u->stream), "event") &&
                  check(hipStreamSynchronize(u->stream), "slice");  // (the staging buffers and the host vectors are free again)
        float ms = 0;
        if (ok && hipEventElapsedTime(&ms, u->ev[0], u->ev[1]) == hipSuccess) u->stats.ms_kmers += ms;
        if (ok && hipEventElapsedTime(&ms, u->ev[1], u->ev[2]) == hipSuccess) u->stats.ms_lookup += ms;
    }
    if (check.rc != GS_OK) {
        u->failed = true;
        return check.rc;
    }
    u64 cnt[2] = {0, 0};
    HIP_TRY(hipMemcpy(cnt, u->d_cnt + 1, sizeof(cnt), hipMemcpyDeviceToHost));
    u->stats.n_pairs = (int64_t)cnt[0];
    u->stats.n_found = (int64_t)cnt[1];
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbupdate_finish(gs_dbupdate *u, int64_t *n_moved) try {
    if (!u || !n_moved) return fail(GS_E_INVALID, "NULL argument");
    if (u->failed) return fail(GS_E_STATE, "an earlier gs_dbupdate_add failed on the device: the values are half-updated (start over)");
    if (u->finished) {
        *n_moved = u->n_moved;
        return GS_OK;
    }
    *n_moved = 0;
    HIP_TRY(hipSetDevice(u->device));
    const auto t0 = std::chrono::steady_clock::now();
    u64 moved = 0;
    HIP_TRY(hipMemsetAsync(u->d_cnt + 3, 0, sizeof(u64), u->stream));
    HIP_TRY(gs_launch_update_moved(u->d_vals, u->d_vals0, u->n, u->d_cnt + 3, u->n_cu, u->stream));
    HIP_TRY(hipMemcpyAsync(&moved, u->d_cnt + 3, sizeof(u64), hipMemcpyDeviceToHost, u->stream));
    HIP_TRY(hipStreamSynchronize(u->stream));
    // the slice's working memory goes (gs_dbupdate_to_db needs the room); batch_bytes_peak keeps what it was
    region_stage_drop_staging(u);
    for (void *p : {(void *)u->d_node, (void *)u->d_pkeys, (void *)u->d_pvals}) gs_dev_free(p);
    u->d_node = nullptr;
    u->d_pkeys = nullptr;
    u->d_pvals = nullptr;
    u->node_cap = u->pair_cap = 0;
    u->n_moved = (int64_t)moved;
    u->stats.n_moved = u->n_moved;
    u->stats.ms_finish = ms_since(t0);
    u->finished = true;
    *n_moved = u->n_moved;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbupdate_fetch(gs_dbupdate *u, int64_t *kmers, int32_t *value_idx) {
    if (!u || (u->n > 0 && (!kmers || !value_idx))) return fail(GS_E_INVALID, "NULL argument");
    if (!u->finished) return fail(GS_E_STATE, "gs_dbupdate_finish first");
    return sorted_store_fetch(u->device, u->n, u->d_keys, u->d_vals, kmers, value_idx);
}

extern "C" int gs_dbupdate_to_db(gs_dbupdate *u, gs_db **out) try {
    if (!u || !out) return fail(GS_E_INVALID, "NULL argument");
    *out = nullptr;
    if (!u->finished) return fail(GS_E_STATE, "gs_dbupdate_finish first");
    return sorted_store_to_db(u->device, u->k, u->n_values, u->parent, u->n, u->d_keys, u->d_vals, "gs_dbupdate_to_db", out);
}
GS_API_CATCH

extern "C" int gs_dbupdate_get_stats(gs_dbupdate *u, gs_dbupdate_stats *out) {
    if (!u || !out) return fail(GS_E_INVALID, "NULL argument");
    *out = u->stats;
    if (!u->finished && !u->failed && u->n > 0) {  // n_moved so far
        if (hipSetDevice(u->device) != hipSuccess) return fail(GS_E_HIP, "hipSetDevice");
        u64 moved = 0;
        HIP_TRY(hipMemsetAsync(u->d_cnt + 3, 0, sizeof(u64), u->stream));
        HIP_TRY(gs_launch_update_moved(u->d_vals, u->d_vals0, u->n, u->d_cnt + 3, u->n_cu, u->stream));
        HIP_TRY(hipMemcpyAsync(&moved, u->d_cnt + 3, sizeof(u64), hipMemcpyDeviceToHost, u->stream));
        HIP_TRY(hipStreamSynchronize(u->stream));
        out->n_moved = (int64_t)moved;
    }
    return GS_OK;
}

extern "C" int gs_dbupdate_destroy(gs_dbupdate *u) {
    if (u) dbupdate_free(u);
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// A collection sized before it is built (gs_size.hip; include/gsgpu.h "gs_dbsize")
// ---------------------------------------------------------------------------------------------------
struct gs_dbsize : RegionStage {
    int n_cu = 256;
    int hb = 1, radix_bits = 0;  // hb = min(hist_bits, 2k)
    bool keep = false;
    u64 range_lo = 0, range_hi = ~0ULL;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // the counter block: total, dust, included, keys retained, distinct; then per_value[n_values]; then hist[1 << hb]
    u64 *d_cnt = nullptr;
    size_t n_cnt = 0;
    u64 *d_buckets = nullptr;  // 1 << radix_bits (a keeping handle with radix_bits > 0)
    int32_t *d_tag = nullptr;
    size_t tag_cap = 0;
    u64 *d_keys = nullptr;  // the retained keys of this pass
    size_t key_cap = 0, n_keys = 0;
    int64_t n_adds = 0;      // of this pass
    bool read = false;       // a counts / distinct since the last add: gs_dbsize_set_range may start the next pass
    bool distinct_done = false;
    bool failed = false;     // a device error in the middle of a call (sticky GS_E_STATE)
    int64_t n_distinct = 0;
    gs_dbsize_stats stats{};
};
enum { GS_SIZE_TOTALS = 0, GS_SIZE_NKEYS = 3, GS_SIZE_NDISTINCT = 4, GS_SIZE_HEAD = 5 };

static void dbsize_free(gs_dbsize *s) {
    region_stage_free(s, {s->d_cnt, s->d_buckets, s->d_tag, s->d_keys});
    for (hipEvent_t e : s->ev)
        if (e) hipEventDestroy(e);
    delete s;
}

static const char *const DBSIZE_FAILED = "an earlier gs_dbsize call failed on the device: the counters are incomplete (start over)";

// every counter of the pass back to zero
static hipError_t dbsize_clear(gs_dbsize *s) {
    hipError_t e = hipMemsetAsync(s->d_cnt, 0, s->n_cnt * sizeof(u64), s->stream);
    if (e == hipSuccess && s->d_buckets) e = hipMemsetAsync(s->d_buckets, 0, sizeof(u64) << s->radix_bits, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    return e;
}

static void dbsize_peak(gs_dbsize *s, size_t sort_bytes) {
    s->stats.bytes_peak = std::max(s->stats.bytes_peak, (int64_t)(s->key_cap * sizeof(u64) + sort_bytes));
}

extern "C" int gs_dbsize_begin(gs_dbsize **out, int device, int k, int32_t n_values, int lower_case_bases, int max_dust, int step_size,
                               int hist_bits, int radix_bits, int keep_keys) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (n_values < 1 || n_values > (1 << 24)) return fail(GS_E_INVALID, "n_values must be in [1, 2^24]");
    // (no upper limit on max_dust here: a score can exceed Short.MAX_VALUE -- (AC)^15 A scores fib(29) -- and a sizing pass may
    // ask what a gate at such a score would drop; the builder's begin refuses it with the reference)
    int rc = region_scan_check(std::min(max_dust, 32767), step_size);
    if (rc) return rc;
    if (hist_bits < 1 || hist_bits > 12) return fail(GS_E_INVALID, "hist_bits must be in [1,12]");
    if (radix_bits != 0 && (radix_bits < 16 || radix_bits > 24)) return fail(GS_E_INVALID, "radix_bits must be 0 or in [16,24] (GSConfigKey.RADIX_STORE_BITS)");
    rc = use_device(device);
    if (rc) return rc;
    gs_dbsize *s = new gs_dbsize();
    rc = region_stage_open(s, device, k, n_values, nullptr, nullptr, lower_case_bases, max_dust, step_size, "gs_dbsize");
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) s->n_cu = cu;
    s->hb = std::min(hist_bits, 2 * k);
    s->keep = keep_keys != 0;
    s->radix_bits = s->keep ? radix_bits : 0;
    s->n_cnt = GS_SIZE_HEAD + (size_t)n_values + ((size_t)1 << s->hb);
    if (!rc) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&s->ev[i]);
        if (e == hipSuccess) e = gs_dev_alloc(&s->d_cnt, s->n_cnt * sizeof(u64));
        if (e == hipSuccess && s->radix_bits > 0) e = gs_dev_alloc(&s->d_buckets, sizeof(u64) << s->radix_bits);
        if (e == hipSuccess) e = dbsize_clear(s);
        if (e != hipSuccess) rc = hip_fail(e, "gs_dbsize_begin");
    }
    if (rc) {
        dbsize_free(s);
        return rc;
    }
    s->stats.bytes_fixed = (int64_t)(s->n_cnt * sizeof(u64) + (s->d_buckets ? sizeof(u64) << s->radix_bits : 0));
    s->stats.n_values = n_values;
    s->stats.hist_bins = 1 << s->hb;
    s->stats.radix_bits = s->radix_bits;
    s->stats.keep_keys = s->keep ? 1 : 0;
    *out = s;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbsize_set_range(gs_dbsize *s, uint64_t lo, uint64_t hi) {
    if (!s || lo >= hi) return fail(GS_E_INVALID, "bad range");
    if (s->failed) return fail(GS_E_STATE, DBSIZE_FAILED);
    if (s->n_adds > 0 && !s->read) return fail(GS_E_STATE, "gs_dbsize_set_range comes before the first gs_dbsize_add, or after gs_dbsize_counts / gs_dbsize_distinct");
    if (s->n_adds > 0 || s->distinct_done) {  // the next pass
        HIP_TRY(hipSetDevice(s->device));
        const hipError_t e = dbsize_clear(s);
        if (e != hipSuccess) {
            s->failed = true;
            return hip_fail(e, "gs_dbsize_set_range");
        }
        s->n_keys = 0;
        s->n_adds = 0;
        s->n_distinct = 0;
        s->read = s->distinct_done = false;
        s->stats.n_bases = s->stats.n_regions = s->stats.n_keys = s->stats.n_distinct = 0;
        s->stats.ms_add = s->stats.ms_count = s->stats.ms_sort = s->stats.ms_heads = 0;
    }
    s->range_lo = lo;
    s->range_hi = hi;
    return GS_OK;
}

extern "C" int gs_dbsize_add(gs_dbsize *s, const uint8_t *seq, const uint64_t *offsets, const int32_t *tag_vi, int64_t n_regions, int mem) try {
    if (!s || n_regions < 0 || (n_regions > 0 && (!seq || !offsets || !tag_vi))) return fail(GS_E_INVALID, "bad argument");
    if (s->failed) return fail(GS_E_STATE, DBSIZE_FAILED);
    if (s->distinct_done) return fail(GS_E_STATE, "gs_dbsize_distinct has released the keys of this pass: gs_dbsize_set_range starts the next one");
    if (n_regions == 0) return GS_OK;
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HIP_TRY(hipSetDevice(s->device));
    for (int64_t r = 0; r < n_regions; r++)
        if (tag_vi[r] < 0 || tag_vi[r] >= s->n_values) return fail(GS_E_INVALID, "tag_vi: not a value index");
    std::vector<uint64_t> hoff;
    int64_t total = 0;
    int rc = region_batch_check(offsets, n_regions, mem, hoff, &total);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    // all of the call's memory before any of its work: an out-of-memory leaves the counters and the keys as they were
    const uint8_t *d_seq = nullptr;
    const u64 *d_off = nullptr;
    {
        HIP_TRY(hipStreamSynchronize(s->stream));
        hipError_t e = mem == GS_MEM_HOST ? dbupdate_room(&s->d_seq, &s->seq_cap, (size_t)std::max<int64_t>(total, 1)) : hipSuccess;
        if (e == hipSuccess && mem == GS_MEM_HOST) e = dbupdate_room(&s->d_off, &s->off_cap, (size_t)n_regions + 1);
        if (e == hipSuccess) e = dbupdate_room(&s->d_tag, &s->tag_cap, (size_t)n_regions);
        if (e == hipSuccess && s->keep && s->n_keys + (size_t)total > s->key_cap) {
            // a slot per position of the batch behind the keys so far; half again while the buffer grows call by call
            const size_t want = std::max(s->n_keys + (size_t)total, s->n_keys ? s->key_cap + s->key_cap / 2 : 0);
            u64 *nk = nullptr;
            e = gs_dev_alloc(&nk, want * sizeof(u64));
            if (e == hipSuccess && s->n_keys) e = hipMemcpyAsync(nk, s->d_keys, s->n_keys * sizeof(u64), hipMemcpyDeviceToDevice, s->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
            if (e == hipSuccess) {
                gs_dev_free(s->d_keys);
                s->d_keys = nk;
                s->key_cap = want;
            } else
                gs_dev_free(nk);
        }
        if (e != hipSuccess) return hip_fail(e, "gs_dbsize_add");
        const int64_t bytes = (int64_t)(s->seq_cap + s->off_cap * sizeof(u64) + s->tag_cap * sizeof(int32_t));
        s->stats.batch_bytes_peak = std::max(s->stats.batch_bytes_peak, bytes);
        dbsize_peak(s, 0);
    }
    GsSizeParams P{};
    P.tag = s->d_tag;
    P.n_regions = n_regions;
    P.total = total;
    P.k = s->k;
    P.lower = s->lower;
    P.step = s->step;
    P.max_dust = s->max_dust;
    P.hist_shift = 2 * s->k - s->hb;
    P.hist_bins = 1 << s->hb;
    P.range_lo = s->range_lo;
    P.range_hi = s->range_hi;
    P.totals = s->d_cnt + GS_SIZE_TOTALS;
    P.per_value = s->d_cnt + GS_SIZE_HEAD;
    P.hist = s->d_cnt + GS_SIZE_HEAD + s->n_values;
    P.keys = s->keep ? s->d_keys : nullptr;
    P.n_keys = s->d_cnt + GS_SIZE_NKEYS;
    P.keys_cap = s->key_cap;
    HipSteps check{"gs_dbsize_add"};
    u64 have = 0;
    rc = region_stage_upload(s, seq, offsets, n_regions, total, mem, &d_seq, &d_off);
    P.seq = d_seq;
    P.off = d_off;
    const bool ok = !rc && check(hipMemcpyAsync(s->d_tag, tag_vi, sizeof(int32_t) * (size_t)n_regions, hipMemcpyHostToDevice, s->stream), "copy") &&
                    check(hipEventRecord(s->ev[0], s->stream), "event") && check(gs_launch_size_count(&P, s->n_cu, s->stream), "count") &&
                    check(hipEventRecord(s->ev[1], s->stream), "event") &&
                    check(hipMemcpyAsync(&have, s->d_cnt + GS_SIZE_NKEYS, sizeof(u64), hipMemcpyDeviceToHost, s->stream), "counter") &&
                    check(hipStreamSynchronize(s->stream), "count");  // (the caller's arrays and the staging buffers are free again)
    if (!ok || have < s->n_keys || have > s->key_cap) {
        s->failed = true;
        return rc ? rc : check.rc != GS_OK ? check.rc : fail(GS_E_HIP, "gs_dbsize_add: key counter out of range");
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->stats.ms_count += ms;
    s->n_keys = (size_t)have;
    s->n_adds++;
    s->read = false;
    s->stats.n_bases += total;
    s->stats.n_regions += n_regions;
    s->stats.n_keys = (int64_t)s->n_keys;
    s->stats.ms_add += ms_since(t0);
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbsize_counts(gs_dbsize *s, gs_dbsize_totals *t, int64_t *per_value, int64_t *hist) try {
    if (!s || !t) return fail(GS_E_INVALID, "NULL argument");
    if (s->failed) return fail(GS_E_STATE, DBSIZE_FAILED);
    HIP_TRY(hipSetDevice(s->device));
    std::vector<u64> h(s->n_cnt);
    HIP_TRY(hipMemcpyAsync(h.data(), s->d_cnt, s->n_cnt * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    t->total = (int64_t)h[GS_SIZE_TOTALS];
    t->dust = (int64_t)h[GS_SIZE_TOTALS + 1];
    t->included = (int64_t)h[GS_SIZE_TOTALS + 2];
    if (per_value) memcpy(per_value, h.data() + GS_SIZE_HEAD, sizeof(int64_t) * (size_t)s->n_values);
    if (hist) memcpy(hist, h.data() + GS_SIZE_HEAD + s->n_values, sizeof(int64_t) << s->hb);
    s->read = true;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbsize_distinct(gs_dbsize *s, int64_t *n_distinct, int64_t *bucket_sizes) try {
    if (!s || !n_distinct) return fail(GS_E_INVALID, "NULL argument");
    if (s->failed) return fail(GS_E_STATE, DBSIZE_FAILED);
    if (!s->keep) return fail(GS_E_STATE, "this handle keeps no keys (gs_dbsize_begin with keep_keys = 0): it counts only");
    if (s->radix_bits > 0 && !bucket_sizes) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->distinct_done) {
        const int64_t n = (int64_t)s->n_keys;
        region_stage_drop_staging(s);
        gs_dev_free(s->d_tag);
        s->d_tag = nullptr;
        s->tag_cap = 0;
        u64 *alt = nullptr, *sorted = nullptr, cnt = 0;
        void *tmp = nullptr;
        size_t tmp_bytes = 0;
        HipSteps check{"gs_dbsize_distinct"};
        auto t0 = std::chrono::steady_clock::now();
        bool ok = true;
        if (n > 0) {
            ok = check(gs_size_sort_bytes(n, 2 * s->k, &tmp_bytes), "sort") && check(gs_dev_alloc(&alt, (size_t)n * sizeof(u64)), "sort buffers") &&
                 check(gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1)), "sort buffers");
            if (ok) dbsize_peak(s, (size_t)n * sizeof(u64) + tmp_bytes);
            ok = ok && check(gs_size_sort(s->d_keys, alt, n, 2 * s->k, tmp, tmp_bytes, &sorted, s->stream), "sort") &&
                 check(hipStreamSynchronize(s->stream), "sort");
            s->stats.ms_sort = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            ok = ok && check(gs_launch_size_heads(sorted, n, s->radix_bits, s->d_cnt + GS_SIZE_NDISTINCT, s->d_buckets, s->n_cu, s->stream), "heads");
        }
        ok = ok && check(hipMemcpyAsync(&cnt, s->d_cnt + GS_SIZE_NDISTINCT, sizeof(u64), hipMemcpyDeviceToHost, s->stream), "heads") &&
             check(hipStreamSynchronize(s->stream), "heads");
        s->stats.ms_heads = n > 0 ? ms_since(t0) : 0;
        gs_dev_free(alt);
        gs_dev_free(tmp);
        gs_dev_free(s->d_keys);  // the retained keys go here
        s->d_keys = nullptr;
        s->key_cap = s->n_keys = 0;
        if (!ok) {
            s->failed = true;
            return check.rc;
        }
        s->n_distinct = (int64_t)cnt;
        s->stats.n_distinct = s->n_distinct;
        s->distinct_done = true;
    }
    *n_distinct = s->n_distinct;
    if (s->radix_bits > 0) HIP_TRY(hipMemcpy(bucket_sizes, s->d_buckets, sizeof(u64) << s->radix_bits, hipMemcpyDeviceToHost));
    s->read = true;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_dbsize_get_stats(gs_dbsize *s, gs_dbsize_stats *out) {
    if (!s || !out) return fail(GS_E_INVALID, "NULL argument");
    *out = s->stats;
    return GS_OK;
}

extern "C" int gs_dbsize_destroy(gs_dbsize *s) {
    if (s) dbsize_free(s);
    return GS_OK;
}

// host arithmetic only: maximal greedy runs of consecutive bins whose sum stays within max_pairs
extern "C" int gs_dbsize_plan(const int64_t *hist, int hist_bits, int k, int64_t max_pairs, uint64_t *bounds, int cap, int *n_ranges) try {
    if (!hist || !bounds || !n_ranges) return fail(GS_E_INVALID, "NULL argument");
    *n_ranges = 0;
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (hist_bits < 1 || hist_bits > 12) return fail(GS_E_INVALID, "hist_bits must be in [1,12]");
    if (max_pairs < 1 || cap < 1) return fail(GS_E_INVALID, "max_pairs and cap must be >= 1");
    const int hb = std::min(hist_bits, 2 * k), shift = 2 * k - hb;
    const int64_t bins = (int64_t)1 << hb;
    int n = 0;
    int64_t sum = 0;
    bounds[0] = 0;
    for (int64_t b = 0; b < bins; b++) {
        const int64_t h = hist[b];
        if (h < 0) return fail(GS_E_INVALID, "gs_dbsize_plan: bin " + std::to_string(b) + " is negative");
        if (h > max_pairs)
            return fail(GS_E_INVALID, "gs_dbsize_plan: bin " + std::to_string(b) + " holds " + std::to_string(h) + " k-mers, more than max_pairs = " +
                                          std::to_string(max_pairs) + ": no range of bins fits (more hist_bits split it)");
        if (sum + h > max_pairs) {  // the run ends in front of this bin
            if (n + 1 >= cap) return fail(GS_E_INVALID, "gs_dbsize_plan: more than cap = " + std::to_string(cap) + " ranges");
            bounds[++n] = (uint64_t)b << shift;
            sum = 0;
        }
        sum += h;
    }
    bounds[++n] = (uint64_t)1 << (2 * k);
    *n_ranges = n;
    return GS_OK;
}
GS_API_CATCH

// ---- Genome FASTA text to regions (gs_genomes.hip; include/gsgpu.h "gs_genomes"): the text work in front of the region stage.
// A handle owns its stream and every buffer; the text is copied into its own padded buffer, so the caller's is free on return.
struct gs_genomes {
    int device = 0;
    hipStream_t stream = nullptr;
    int state = 0;  // 0: no chunk; 1: scanned; 2: gathered
    uint8_t *d_text = nullptr;
    size_t text_cap = 0;
    u64 *d_tile = nullptr;  // tile_hl | tile_c, tile_cap entries each
    size_t tile_cap = 0;
    uint32_t *d_line = nullptr;  // nl | cnl, line_cap entries each
    size_t line_cap = 0;
    uint32_t *d_rec32 = nullptr;  // rec_start | rec_line | base_start | base_cnt, rec_cap entries each
    u64 *d_rec64 = nullptr;       // hdr_off | sel | off | rec_block, rec_cap entries each
    uint8_t *d_keep = nullptr;
    size_t rec_cap = 0;
    uint8_t *d_hdr = nullptr, *d_seq = nullptr;
    size_t hdr_cap = 0, seq_cap = 0;
    u64 *d_small = nullptr;  // status (GS_GN_WORDS words of 32 bits), res
    int last = 0;
    int64_t n_bytes = 0, n_tiles = 0, n_hdr = 0, n_nl = 0, n_records = 0, cut = 0, hdr_bytes = 0, max_line = 0, n_kept = 0, n_bases = 0;
    KernelTimer t_scan, t_gather;
};
enum { GN_S_STATUS = 0, GN_S_RES = GS_GN_WORDS / 2, GN_S_WORDS = GN_S_RES + GS_GN_R_WORDS };

static void gn_params(gs_genomes *g, GsGenomesParams *P) {
    P->text = g->d_text;
    P->n_bytes = g->n_bytes;
    P->n_tiles = g->n_tiles;
    P->last = g->last;
    P->tile_hl = (unsigned long long *)g->d_tile;
    P->tile_c = (unsigned long long *)g->d_tile + g->tile_cap;
    P->status = (uint32_t *)(g->d_small + GN_S_STATUS);
    P->res = (unsigned long long *)g->d_small + GN_S_RES;
    P->n_hdr = g->n_hdr;
    P->n_nl = g->n_nl;
    P->n_records = g->n_records;
    P->nl = g->d_line;
    P->cnl = g->d_line + g->line_cap;
    P->rec_start = g->d_rec32;
    P->rec_line = g->d_rec32 + g->rec_cap;
    P->base_start = g->d_rec32 + 2 * g->rec_cap;
    P->base_cnt = g->d_rec32 + 3 * g->rec_cap;
    P->hdr_off = (unsigned long long *)g->d_rec64;
    P->sel = (unsigned long long *)g->d_rec64 + g->rec_cap;
    P->off = (unsigned long long *)g->d_rec64 + 2 * g->rec_cap;
    P->rec_block = (unsigned long long *)g->d_rec64 + 3 * g->rec_cap;
    P->hdr_out = g->d_hdr;
    P->keep = nullptr;
    P->seq = g->d_seq;
}

extern "C" int gs_genomes_destroy(gs_genomes *g) {
    if (!g) return GS_OK;
    hipSetDevice(g->device);
    if (g->stream) hipStreamSynchronize(g->stream);
    timer_free(g->t_scan);
    timer_free(g->t_gather);
    for (void *p : {(void *)g->d_text, (void *)g->d_tile, (void *)g->d_line, (void *)g->d_rec32, (void *)g->d_rec64, (void *)g->d_keep, (void *)g->d_hdr,
                    (void *)g->d_seq, (void *)g->d_small})
        gs_dev_free(p);
    if (g->stream) hipStreamDestroy(g->stream);
    delete g;
    return GS_OK;
}

extern "C" int gs_genomes_create(gs_genomes **out, int device) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (device < 0) return fail(GS_E_INVALID, "device index out of range");
    int rc = use_device(device);
    if (rc) return rc;
    gs_genomes *g = new gs_genomes();
    g->device = device;
    hipError_t e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc(&g->d_small, sizeof(u64) * GN_S_WORDS);
    if (e != hipSuccess) {
        gs_genomes_destroy(g);
        return hip_fail(e, "gs_genomes_create");
    }
    *out = g;
    return GS_OK;
}
GS_API_CATCH

// the buffers grow by doubling: a collection's chunks are of one size, its records are not
template <typename T>
static int gn_grow(T **p, size_t *cap, size_t need, size_t arrays, hipStream_t stream) {
    if (*cap >= need) return GS_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    *cap = 0;
    const int rc = renew(p, 2 * need * arrays);
    if (!rc) *cap = 2 * need;
    return rc;
}

// the per-record arrays, all of one capacity
static int gn_record_room(gs_genomes *g, size_t need) {
    if (g->rec_cap >= need) return GS_OK;
    int rc = gn_grow(&g->d_rec32, &g->rec_cap, need, 4, g->stream);
    if (!rc) rc = renew(&g->d_rec64, 4 * g->rec_cap);
    if (!rc) rc = renew(&g->d_keep, g->rec_cap);
    if (rc) g->rec_cap = 0;
    return rc;
}

extern "C" int gs_genomes_scan(gs_genomes *g, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t *n_records, int64_t *consumed_bytes,
                               int64_t *header_bytes, int64_t *max_line_bytes) try {
    if (!g) return fail(GS_E_INVALID, "genomes is NULL");
    if (n_bytes < 0 || (n_bytes > 0 && !text)) return fail(GS_E_INVALID, "text is NULL or n_bytes is negative");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (!n_records || !consumed_bytes || !header_bytes || !max_line_bytes) return fail(GS_E_INVALID, "NULL output argument");
    *n_records = *consumed_bytes = *header_bytes = *max_line_bytes = 0;
    g->state = 0;
    if (n_bytes > ((int64_t)1 << 30)) return fail(GS_E_UNSUPPORTED, "a chunk holds at most 1 GiB: a record that does not fit is the host parser's");
    HIP_TRY(hipSetDevice(g->device));
    g->n_bytes = n_bytes;
    g->n_tiles = (n_bytes + GS_GN_TILE - 1) / GS_GN_TILE;
    g->last = last != 0;
    g->n_hdr = g->n_nl = g->n_records = g->cut = g->hdr_bytes = g->max_line = g->n_kept = g->n_bases = 0;
    int rc;
    if ((rc = gn_record_room(g, 1))) return rc;  // (a chunk without records still has off[0])
    if (n_bytes == 0) {
        g->state = 1;
        return GS_OK;
    }
    const size_t padded = (size_t)g->n_tiles * GS_GN_TILE + GS_GN_PAD;
    if ((rc = gn_grow(&g->d_text, &g->text_cap, padded, 1, g->stream))) return rc;
    if ((rc = gn_grow(&g->d_tile, &g->tile_cap, (size_t)g->n_tiles + 1, 2, g->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(g->d_text, text, (size_t)n_bytes, mem == GS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, g->stream));
    HIP_TRY(hipMemsetAsync(g->d_text + n_bytes, '\n', padded - (size_t)n_bytes, g->stream));
    HIP_TRY(hipMemsetAsync(g->d_small, 0, sizeof(u64) * GN_S_WORDS, g->stream));
    HIP_TRY(hipMemsetAsync(g->d_small + GN_S_STATUS, 0xff, 2 * sizeof(uint32_t), g->stream));  // GS_GN_NUL, GS_GN_CR: none
    GsGenomesParams P{};
    gn_params(g, &P);
    if ((rc = timer_start(g->t_scan, true, g->stream))) return rc;
    HIP_TRY(gs_launch_genomes_count(&P, g->stream));
    if ((rc = timer_stop(g->t_scan, true, g->stream))) return rc;
    uint32_t status[GS_GN_WORDS];
    u64 sums[2];
    HIP_TRY(hipMemcpyAsync(status, g->d_small + GN_S_STATUS, sizeof(status), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&sums[0], P.tile_hl + g->n_tiles, sizeof(u64), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(&sums[1], P.tile_c + g->n_tiles, sizeof(u64), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));  // (the caller's text is free again)
    if (status[GS_GN_NUL] != 0xffffffffu || status[GS_GN_CR] != 0xffffffffu) {
        const bool nul = status[GS_GN_NUL] < status[GS_GN_CR];
        return fail(GS_E_UNSUPPORTED, std::string("gs_genomes_scan: ") + (nul ? "a NUL byte" : "a run of more than " + std::to_string(GS_GN_CR_CAP) + " '\\r'") +
                                          " at byte offset " + std::to_string(nul ? status[GS_GN_NUL] : status[GS_GN_CR]) + ": this chunk is the host parser's");
    }
    g->n_hdr = (int64_t)(sums[0] >> 32);
    g->n_nl = (int64_t)(sums[0] & 0xffffffffu);
    if (g->n_hdr >= GS_GN_MAX_RECORDS)  // (the selection scan keeps the kept records in the 24 bits above bit 40)
        return fail(GS_E_UNSUPPORTED, "gs_genomes_scan: " + std::to_string((long long)g->n_hdr) + " header lines in one chunk: at most 2^24 - 1 (cut the chunk)");
    g->n_records = g->last ? g->n_hdr : std::max<int64_t>(g->n_hdr - 1, 0);
    if ((rc = gn_grow(&g->d_line, &g->line_cap, (size_t)g->n_nl + 1, 2, g->stream))) return rc;
    if ((rc = gn_record_room(g, (size_t)g->n_hdr + 1))) return rc;
    gn_params(g, &P);
    if ((rc = timer_start(g->t_scan, true, g->stream))) return rc;
    HIP_TRY(gs_launch_genomes_records(&P, g->stream));
    if ((rc = timer_stop(g->t_scan, true, g->stream))) return rc;
    u64 res[GS_GN_R_WORDS];
    HIP_TRY(hipMemcpyAsync(status, g->d_small + GN_S_STATUS, sizeof(status), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(res, g->d_small + GN_S_RES, sizeof(res), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if ((rc = timer_collect(g->t_scan))) return rc;
    g->cut = (int64_t)res[GS_GN_R_CUT];
    g->hdr_bytes = (int64_t)res[GS_GN_R_HDR_BYTES];
    g->max_line = status[GS_GN_MAXLINE];
    g->state = 1;
    *n_records = g->n_records;
    *consumed_bytes = g->cut;
    *header_bytes = g->hdr_bytes;
    *max_line_bytes = g->max_line;
    return GS_OK;
}
GS_API_CATCH

// the header lines of the scanned chunk back to back in g->d_hdr, P->hdr_off[n_records + 1] beside them (g->n_records > 0); the
// stream has the work, nothing waits for it
static int gn_device_headers(gs_genomes *g, GsGenomesParams *P) {
    HIP_TRY(hipSetDevice(g->device));
    int rc = gn_grow(&g->d_hdr, &g->hdr_cap, (size_t)std::max<int64_t>(g->hdr_bytes, 1), 1, g->stream);
    if (rc) return rc;
    gn_params(g, P);
    HIP_TRY(gs_launch_genomes_headers(P, g->stream));
    return GS_OK;
}

extern "C" int gs_genomes_headers(gs_genomes *g, uint8_t *headers, uint64_t *header_off) try {
    if (!g || !header_off) return fail(GS_E_INVALID, "NULL argument");
    if (g->state < 1) return fail(GS_E_STATE, "gs_genomes_headers comes behind a gs_genomes_scan that took its chunk");
    if (g->hdr_bytes > 0 && !headers) return fail(GS_E_INVALID, "headers is NULL");
    header_off[0] = 0;
    if (g->n_records == 0) return GS_OK;
    GsGenomesParams P{};
    int rc = gn_device_headers(g, &P);
    if (rc) return rc;
    if (g->hdr_bytes > 0) HIP_TRY(hipMemcpyAsync(headers, g->d_hdr, (size_t)g->hdr_bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(header_off, P.hdr_off, sizeof(u64) * ((size_t)g->n_records + 1), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_genomes_gather(gs_genomes *g, const uint8_t *keep, int64_t *n_regions, int64_t *n_bases) try {
    if (!g || !n_regions || !n_bases) return fail(GS_E_INVALID, "NULL argument");
    *n_regions = *n_bases = 0;
    if (g->state < 1) return fail(GS_E_STATE, "gs_genomes_gather comes behind a gs_genomes_scan that took its chunk");
    HIP_TRY(hipSetDevice(g->device));
    g->state = 1;
    g->n_kept = g->n_bases = 0;
    GsGenomesParams P{};
    gn_params(g, &P);
    int rc;
    if (g->n_records == 0) {
        HIP_TRY(hipMemsetAsync(P.off, 0, sizeof(u64), g->stream));
    } else {
        if (keep) {
            HIP_TRY(hipMemcpyAsync(g->d_keep, keep, (size_t)g->n_records, hipMemcpyHostToDevice, g->stream));
            P.keep = g->d_keep;
        }
        HIP_TRY(hipMemsetAsync(P.res + GS_GN_R_KEPT, 0, sizeof(u64), g->stream));
        if ((rc = timer_start(g->t_gather, true, g->stream))) return rc;
        HIP_TRY(gs_launch_genomes_select(&P, g->stream));
        if ((rc = timer_stop(g->t_gather, true, g->stream))) return rc;
        u64 kept = 0;
        HIP_TRY(hipMemcpyAsync(&kept, P.res + GS_GN_R_KEPT, sizeof(u64), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));  // (the caller's flags are free again)
        g->n_kept = (int64_t)(kept >> 40);
        g->n_bases = (int64_t)(kept & ((1ULL << 40) - 1));
    }
    if ((rc = gn_grow(&g->d_seq, &g->seq_cap, (size_t)g->n_bases + 16, 1, g->stream))) return rc;
    P.seq = g->d_seq;
    if (g->n_bases > 0) {
        if ((rc = timer_start(g->t_gather, true, g->stream))) return rc;
        HIP_TRY(gs_launch_genomes_gather(&P, (g->cut + GS_GN_TILE - 1) / GS_GN_TILE, g->stream));
        if ((rc = timer_stop(g->t_gather, true, g->stream))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(g->stream));  // (the regions are complete: an _add call on its own stream may read them)
    if ((rc = timer_collect(g->t_gather))) return rc;
    g->state = 2;
    *n_regions = g->n_kept;
    *n_bases = g->n_bases;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_genomes_regions(gs_genomes *g, const uint8_t **d_seq, const uint64_t **d_off) {
    if (!g || !d_seq || !d_off) return fail(GS_E_INVALID, "NULL argument");
    if (g->state < 2) return fail(GS_E_STATE, "gs_genomes_regions comes behind gs_genomes_gather");
    *d_seq = g->d_seq;
    *d_off = (const uint64_t *)(g->d_rec64 + 2 * g->rec_cap);
    return GS_OK;
}

extern "C" int gs_genomes_kernel_time(gs_genomes *g, double *ms_scan, double *ms_gather) {
    if (!g || !ms_scan || !ms_gather) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));
    int rc = timer_collect(g->t_scan);
    if (!rc) rc = timer_collect(g->t_gather);
    if (rc) return rc;
    *ms_scan = g->t_scan.total_ms;
    *ms_gather = g->t_gather.total_ms;
    return GS_OK;
}

// ---- DB-partitioned mode: encode / probe / reduce as separate steps (all pointers are device pointers)
extern "C" int gs_match_encode(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                               const uint64_t *pos_off, uint64_t *keys) {
    if (!run || (n_reads > 0 && (!seq || !offsets || !pos_off || !keys))) return fail(GS_E_INVALID, "NULL argument");
    if (run->db->n_rec > 0) return fail(GS_E_STATE, "the split pipeline needs a partition store (gs_db_create_part): this store keeps k-mers in super-k-mer records");
    if (n_reads <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    GsEncodeParams P{};
    P.k = run->db->info.k;
    P.seq = seq;
    P.off = offsets;
    P.n_reads = n_reads;
    P.pos_off = (const unsigned long long *)pos_off;
    P.keys = (unsigned long long *)keys;
    P.mgate = run->db->dev.mgate;
    P.mgate_bits = run->db->dev.mgate_bits;
    int grid = (int)std::min<int64_t>((int64_t)run->db->n_cu * 8, (n_reads + 3) / 4);
    if (grid < 1) grid = 1;
    HIP_TRY(gs_launch_encode(&P, grid, run->stream));
    return GS_OK;
}

static int route_grid(const gs_run *run, int64_t n_reads) {  // workgroups of GS_BLOCK / 64 waves (one read per wave at a time)
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)run->db->n_cu * 8, (n_reads + 3) / 4));
}

extern "C" int gs_match_route_geometry(const gs_run *run, int64_t n_reads, int32_t *n_waves, int32_t *chunk) {
    if (!run || n_reads < 0) return fail(GS_E_INVALID, "bad argument");
    if (n_waves) *n_waves = route_grid(run, n_reads) * (GS_BLOCK / 64);
    if (chunk) *chunk = GS_ROUTE_CHUNK;
    return GS_OK;
}

extern "C" int gs_match_encode_route(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, const uint64_t *pos_off,
                                     int n_parts, int64_t cap, uint64_t *send_keys, uint32_t *send_idx, int32_t *nodes,
                                     int64_t *counts, int *overflow) {
    if (!run || !counts || !overflow || n_parts < 1 || n_parts > 64 || cap < GS_ROUTE_CHUNK || (cap % GS_ROUTE_CHUNK) != 0 ||
        (n_reads > 0 && (!seq || !offsets || !pos_off || !send_keys || !send_idx || !nodes)))
        return fail(GS_E_INVALID, "bad argument (cap must be a multiple of 2048)");
    if (run->db->n_rec > 0) return fail(GS_E_STATE, "the split pipeline needs a partition store (gs_db_create_part): this store keeps k-mers in super-k-mer records");
    for (int i = 0; i < n_parts; i++) counts[i] = 0;
    *overflow = 0;
    if (n_reads <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    {   // a routed key carries its position in the batch as 32 bits (send_idx, ~0 = unused slot): as gs_route_keys, refuse a batch
        // whose positions do not fit instead of scattering the answers to truncated positions
        u64 n_pos = 0;
        HIP_TRY(hipMemcpyAsync(&n_pos, pos_off + n_reads, sizeof(u64), hipMemcpyDeviceToHost, run->stream));
        HIP_TRY(hipStreamSynchronize(run->stream));
        if (n_pos >= 0xffffffffULL) return fail(GS_E_INVALID, "more than 2^32-2 k-mer positions in one batch: split the batch");
    }
    if (!run->d_route_cursors) HIP_TRY(gs_dev_alloc((void **)&run->d_route_cursors, sizeof(u64) * 65));
    HIP_TRY(hipMemsetAsync(run->d_route_cursors, 0, sizeof(u64) * 65, run->stream));
    GsEncodeParams P{};
    P.k = run->db->info.k;
    P.seq = seq;
    P.off = offsets;
    P.n_reads = n_reads;
    P.pos_off = (const unsigned long long *)pos_off;
    P.keys = nullptr;
    P.mgate = run->db->dev.mgate;
    P.mgate_bits = run->db->dev.mgate_bits;
    GsRouteParams R{};
    R.n_parts = n_parts;
    R.cap = (unsigned long long)cap;
    R.cursors = (unsigned long long *)run->d_route_cursors;
    R.send_keys = (unsigned long long *)send_keys;
    R.send_idx = send_idx;
    R.nodes = nodes;
    HIP_TRY(gs_launch_encode_route(&P, &R, route_grid(run, n_reads), run->stream));
    u64 h[65];
    HIP_TRY(hipMemcpyAsync(h, run->d_route_cursors, sizeof(h), hipMemcpyDeviceToHost, run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    for (int i = 0; i < n_parts; i++) counts[i] = (int64_t)std::min<u64>(h[i], (u64)cap);
    *overflow = h[64] != 0;
    return GS_OK;
}

extern "C" int gs_unroute_region(gs_run *run, const uint32_t *idx, const int32_t *back, int64_t n, int32_t *nodes) {
    if (!run || (n > 0 && (!idx || !back || !nodes))) return fail(GS_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(gs_launch_unroute_region(idx, back, n, nodes, run->stream));
    return GS_OK;
}

extern "C" int gs_match_probe_keys(gs_run *run, const uint64_t *keys, int64_t n_keys, int32_t *nodes) {
    if (!run || (n_keys > 0 && (!keys || !nodes))) return fail(GS_E_INVALID, "NULL argument");
    if (run->db->n_rec > 0) return fail(GS_E_STATE, "the split pipeline needs a partition store (gs_db_create_part): this store keeps k-mers in super-k-mer records");
    if (n_keys <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    if (run->cfg.count_unique) {
        run->seen_dirty = true;
        run->bitmap_merged = false;
    }
    HIP_TRY(gs_launch_probe_keys(&run->db->dev, (const u64 *)keys, n_keys, nodes, run->cfg.count_unique, run->stream));
    return GS_OK;
}

extern "C" int gs_match_reduce(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads,
                               int64_t first_read_no, const uint64_t *pos_off, const int32_t *nodes, int32_t *class_vi,
                               uint8_t *flags) {
    if (!run || (n_reads > 0 && (!seq || !offsets || !pos_off || !nodes))) return fail(GS_E_INVALID, "NULL argument");
    if (n_reads <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    return launch_batch(run, seq, offsets, n_reads, first_read_no, class_vi, flags, nodes, pos_off);
}

// groups the valid keys by owner rank (counting sort on the device); counts[n_parts] is a HOST array
extern "C" int gs_route_keys(gs_run *run, const uint64_t *keys, int64_t n_keys, int n_parts, uint64_t *send_keys,
                             uint32_t *idx, int64_t *counts, int32_t *nodes) {
    if (!run || !counts || n_parts < 1 || n_parts > 64 || (n_keys > 0 && (!keys || !send_keys || !idx)))
        return fail(GS_E_INVALID, "bad argument");
    if (n_keys >= ((int64_t)1 << 32)) return fail(GS_E_INVALID, "more than 2^32-1 keys in one batch");
    HIP_TRY(hipSetDevice(run->db->device));
    for (int i = 0; i < n_parts; i++) counts[i] = 0;
    if (n_keys <= 0) return GS_OK;
    u64 *d_counts = nullptr;
    HIP_TRY(gs_dev_alloc((void **)&d_counts, sizeof(u64) * 64));
    hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(u64) * 64, run->stream);
    if (e == hipSuccess) e = gs_launch_route_count((const u64 *)keys, n_keys, n_parts, d_counts, run->stream);
    u64 h[64];
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_counts, sizeof(u64) * 64, hipMemcpyDeviceToHost, run->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(run->stream);
    u64 cur[64], acc = 0;
    for (int i = 0; i < 64; i++) {
        cur[i] = acc;
        if (i < n_parts) {
            counts[i] = (int64_t)h[i];
            acc += h[i];
        }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_counts, cur, sizeof(u64) * 64, hipMemcpyHostToDevice, run->stream);
    if (e == hipSuccess)
        e = gs_launch_route_scatter((const u64 *)keys, n_keys, n_parts, d_counts, (u64 *)send_keys, idx, nodes, run->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(run->stream);
    gs_dev_free(d_counts);
    if (e != hipSuccess) return fail(GS_E_HIP, std::string("gs_route_keys: ") + hipGetErrorString(e));
    return GS_OK;
}

// inverse of gs_route_keys for the nodes that came back: nodes[idx[i]] = back[i]; unrouted positions read -2 (key ~0)
// or -1 (key ~0 - 1: ruled out by the gate of the encoding rank)
extern "C" int gs_unroute_nodes(gs_run *run, const uint64_t *keys, const uint32_t *idx, const int32_t *back,
                                int64_t n_routed, int32_t *nodes, int64_t n_keys) {
    if (!run || (n_keys > 0 && !nodes) || (n_routed > 0 && (!idx || !back))) return fail(GS_E_INVALID, "bad argument");
    if (n_keys <= 0) return GS_OK;
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(gs_launch_unroute((const u64 *)keys, idx, back, n_routed, nodes, n_keys, run->stream));
    return GS_OK;
}

// ---- Kraken-style segments (two passes: count, host prefix sum, write)
static int stage_batch(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, int mem,
                       const uint8_t **d_seq, const uint64_t **d_off) {
    if (mem == GS_MEM_DEVICE) {
        *d_seq = seq;
        *d_off = offsets;
        return GS_OK;
    }
    if (mem != GS_MEM_HOST) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    // (on the run's stream, like the kernels that read it; segments_core synchronises before it returns, so h.rel is free by then)
    HostStage &h = run->host;
    int rc = stage_room(h, (size_t)(offsets[n_reads] - offsets[0]), (size_t)n_reads, run->stream);
    if (!rc) rc = stage_upload(h, seq, offsets, n_reads, run->stream);
    *d_seq = h.d_seq;
    *d_off = h.d_off;
    return rc;
}

static int segments_core(gs_run *run, const uint8_t *d_seq, const uint64_t *d_off, int64_t n_reads, int off_stride, uint64_t *seg_off) {
    gs_dev_free(run->d_seg_count);
    gs_dev_free(run->d_seg_off);
    gs_dev_free(run->d_seg_code);
    gs_dev_free(run->d_seg_start);
    run->d_seg_count = nullptr;
    run->d_seg_off = nullptr;
    run->d_seg_code = run->d_seg_start = nullptr;
    HIP_TRY(gs_dev_alloc((void **)&run->d_seg_count, sizeof(uint32_t) * (size_t)n_reads));
    HIP_TRY(gs_dev_alloc((void **)&run->d_seg_off, sizeof(u64) * ((size_t)n_reads + 1)));
    GsSegParams P{};
    P.db = run->db->dev;
    P.seq = d_seq;
    P.off = d_off;
    P.off_stride = off_stride;
    P.n_reads = n_reads;
    P.seg_count = run->d_seg_count;
    P.huge_min = GS_HUGE_MIN;
    if (const char *e = getenv("GS_HUGE_MIN")) P.huge_min = std::max(129, atoi(e));
    int grid = (int)std::min<int64_t>(run->grid, (n_reads + 3) / 4);
    if (grid < 1) grid = 1;
    HIP_TRY(gs_launch_segments(&P, 0, grid, run->stream));
    std::vector<uint32_t> counts((size_t)n_reads);
    HIP_TRY(hipMemcpyAsync(counts.data(), run->d_seg_count, sizeof(uint32_t) * (size_t)n_reads, hipMemcpyDeviceToHost,
                           run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    // Reads of tens of thousands of positions and more were left out (one wave would walk a chromosome for 150 ms per pass): they come
    // back in pieces of GS_SEG_PIECE_ITERS iterations, one wave each.  A piece counts its first position as the start of a run; the
    // seams where the node goes on are taken off here, and the write pass gets the node in front of every piece.
    std::vector<GsSegPiece> pieces;
    std::vector<size_t> first_piece;  // per left-out read, + end
    std::vector<int64_t> huge_reads;
    struct Dev {  // (freed on every way out)
        GsSegPiece *pieces = nullptr;
        GsSegPieceOut *out = nullptr;
        ~Dev() {
            gs_dev_free(pieces);
            gs_dev_free(out);
        }
    } dv;
    for (int64_t r = 0; r < n_reads; r++)
        if (counts[(size_t)r] == GS_SEG_HUGE) huge_reads.push_back(r);
    if (!huge_reads.empty()) {
        const int k = run->db->info.k;
        for (int64_t r : huge_reads) {
            uint64_t se[2];
            HIP_TRY(hipMemcpy(se, d_off + r * off_stride, sizeof(se), hipMemcpyDeviceToHost));
            const int64_t max = (int64_t)(se[1] - se[0]) - k + 1, n_iter = (max + 127) >> 7;
            first_piece.push_back(pieces.size());
            for (int64_t it = 0; it < n_iter; it += GS_SEG_PIECE_ITERS) {
                GsSegPiece pc{};
                pc.read = (uint32_t)r;
                pc.it0 = (int32_t)it;
                pc.n_iter = (int32_t)std::min<int64_t>(GS_SEG_PIECE_ITERS, n_iter - it);
                pc.carry = -3;  // GS_NODE_NONE
                pieces.push_back(pc);
            }
        }
        first_piece.push_back(pieces.size());
        HIP_TRY(gs_dev_alloc((void **)&dv.pieces, sizeof(GsSegPiece) * pieces.size()));
        HIP_TRY(gs_dev_alloc((void **)&dv.out, sizeof(GsSegPieceOut) * pieces.size()));
        HIP_TRY(hipMemcpyAsync(dv.pieces, pieces.data(), sizeof(GsSegPiece) * pieces.size(), hipMemcpyHostToDevice, run->stream));
        GsSegParams Q = P;
        Q.pieces = dv.pieces;
        Q.piece_out = dv.out;
        Q.n_pieces = (int64_t)pieces.size();
        const int pgrid = (int)std::max<int64_t>(1, std::min<int64_t>(run->grid, ((int64_t)pieces.size() + 3) / 4));
        HIP_TRY(gs_launch_segments(&Q, 0, pgrid, run->stream));
        std::vector<GsSegPieceOut> outs(pieces.size());
        HIP_TRY(hipMemcpyAsync(outs.data(), dv.out, sizeof(GsSegPieceOut) * pieces.size(), hipMemcpyDeviceToHost, run->stream));
        HIP_TRY(hipStreamSynchronize(run->stream));
        for (size_t h = 0; h < huge_reads.size(); h++) {
            uint64_t total = 0;
            for (size_t i = first_piece[h]; i < first_piece[h + 1]; i++) {
                uint32_t c = outs[i].count;
                if (i > first_piece[h]) {
                    pieces[i].carry = outs[i - 1].last_node;
                    if (outs[i].first_node == outs[i - 1].last_node) c--;  // the run goes on across the seam
                }
                pieces[i].out_off = total;
                total += c;
            }
            if (total >= GS_SEG_HUGE) return fail(GS_E_INVALID, "more than 2^32 - 2 segments in one read");
            counts[(size_t)huge_reads[h]] = (uint32_t)total;
        }
    }
    for (int64_t i = 0; i < n_reads; i++) seg_off[i + 1] = seg_off[i] + counts[(size_t)i];
    run->seg_total = (int64_t)seg_off[n_reads];
    if (run->seg_total > 0) {
        HIP_TRY(gs_dev_alloc((void **)&run->d_seg_code, sizeof(int32_t) * (size_t)run->seg_total));
        HIP_TRY(gs_dev_alloc((void **)&run->d_seg_start, sizeof(int32_t) * (size_t)run->seg_total));
        HIP_TRY(hipMemcpyAsync(run->d_seg_off, seg_off, sizeof(u64) * ((size_t)n_reads + 1), hipMemcpyHostToDevice, run->stream));
        P.seg_off = run->d_seg_off;
        P.seg_code = run->d_seg_code;
        P.seg_start = run->d_seg_start;
        HIP_TRY(gs_launch_segments(&P, 1, grid, run->stream));
        if (!pieces.empty()) {
            HIP_TRY(hipMemcpyAsync(dv.pieces, pieces.data(), sizeof(GsSegPiece) * pieces.size(), hipMemcpyHostToDevice, run->stream));
            GsSegParams Q = P;
            Q.pieces = dv.pieces;
            Q.n_pieces = (int64_t)pieces.size();
            const int pgrid = (int)std::max<int64_t>(1, std::min<int64_t>(run->grid, ((int64_t)pieces.size() + 3) / 4));
            HIP_TRY(gs_launch_segments(&Q, 1, pgrid, run->stream));
        }
        HIP_TRY(hipStreamSynchronize(run->stream));
    }
    return GS_OK;
}

extern "C" int gs_match_segments(gs_run *run, const uint8_t *seq, const uint64_t *offsets, int64_t n_reads, int mem,
                                 uint64_t *seg_off) try {
    if (!run || !seg_off) return fail(GS_E_INVALID, "NULL argument");
    if (n_reads < 0 || (n_reads > 0 && (!seq || !offsets))) return fail(GS_E_INVALID, "bad batch arrays");
    HIP_TRY(hipSetDevice(run->db->device));
    seg_off[0] = 0;
    run->seg_total = 0;
    if (n_reads == 0) return GS_OK;
    const uint8_t *d_seq = nullptr;
    const uint64_t *d_off = nullptr;
    int rc = stage_batch(run, seq, offsets, n_reads, mem, &d_seq, &d_off);
    if (rc) return rc;
    return segments_core(run, d_seq, d_off, n_reads, 1, seg_off);
}
GS_API_CATCH

// the same for the reads of the most recent text chunk (which must not have been refused: gs_match_text_status)
extern "C" int gs_match_segments_text(gs_run *run, uint64_t *seg_off) try {
    if (!run || !seg_off) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    seg_off[0] = 0;
    run->seg_total = 0;
    const int64_t n_reads = run->text.last_reads;
    if (run->text.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    if (n_reads == 0) return GS_OK;
    const bool fasta = run->text.last_fasta;  // (the gathered sequences stay in place until the next FASTA chunk)
    const int rc = segments_core(run, fasta ? run->text.d_fa_seq : run->text.d_text, (const uint64_t *)run->text.d_off2, n_reads,
                                 fasta ? 1 : 2, seg_off);
    if (rc) return rc;
    return text_touched(run->text, run->stream);
}
GS_API_CATCH

// newline offsets of the most recent text chunk (the record geometry for per-read writers); synchronises
extern "C" int gs_match_text_read_bounds(gs_run *run, uint64_t *bounds) {
    if (!run || !bounds) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    const int rc = text_read_bounds(run->text, run->stream, bounds,
                                    "the last chunk was four-line FASTQ: its reads lie in the text (gs_match_text_newlines)");
    return rc ? rc : timer_collect(run->timer);
}

extern "C" int gs_match_text_line_classes(gs_run *run, uint8_t *classes) {
    if (!run || !classes) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    const int rc = text_line_classes(run->text, run->stream, classes);
    return rc ? rc : timer_collect(run->timer);
}

extern "C" int gs_match_text_newlines(gs_run *run, uint32_t *newlines) {
    if (!run || !newlines) return fail(GS_E_INVALID, "NULL argument");
    if (run->text.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    HIP_TRY(hipSetDevice(run->db->device));
    if (run->text.last_lines > 0)
        HIP_TRY(hipMemcpyAsync(newlines, run->text.d_nl, sizeof(uint32_t) * (size_t)run->text.last_lines, hipMemcpyDeviceToHost, run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    return timer_collect(run->timer);
}

extern "C" int gs_match_segments_fetch(gs_run *run, int32_t *codes, int32_t *starts) {
    if (!run || (run->seg_total > 0 && (!codes || !starts))) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    if (run->seg_total > 0) {
        HIP_TRY(hipMemcpy(codes, run->d_seg_code, sizeof(int32_t) * (size_t)run->seg_total, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(starts, run->d_seg_start, sizeof(int32_t) * (size_t)run->seg_total, hipMemcpyDeviceToHost));
    }
    return GS_OK;
}

// ---- Kraken-style lines of a four-line chunk as device text (gs_kraken.hip)
extern "C" int gs_match_set_taxids(gs_run *run, const char *const *taxids) try {
    if (!run || !taxids) return fail(GS_E_INVALID, "NULL argument");
    const size_t nv = (size_t)run->db->info.n_values;
    std::vector<uint32_t> off(nv + 1, 0);
    for (size_t v = 0; v < nv; v++) {
        if (!taxids[v]) return fail(GS_E_INVALID, "NULL taxid string");
        const size_t len = strlen(taxids[v]);
        if (len > 0xffffffffu - off[v]) return fail(GS_E_INVALID, "taxid strings of 4 GiB and more");
        off[v + 1] = off[v] + (uint32_t)len;
    }
    std::vector<uint8_t> bytes((size_t)off[nv] + 1);
    for (size_t v = 0; v < nv; v++) memcpy(bytes.data() + off[v], taxids[v], off[v + 1] - off[v]);
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));  // (nothing reads the earlier set any more)
    int rc = renew(&run->d_tax_bytes, bytes.size());
    if (!rc) rc = renew(&run->d_tax_off, nv + 1);
    if (rc) {
        gs_dev_free(run->d_tax_off);
        run->d_tax_off = nullptr;
        return rc;
    }
    HIP_TRY(hipMemcpy(run->d_tax_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(run->d_tax_off, off.data(), sizeof(uint32_t) * (nv + 1), hipMemcpyHostToDevice));
    return GS_OK;
}
GS_API_CATCH

// records: the last chunk must be FASTA or general FASTQ (gs_match_kraken_records), else four-line FASTQ (gs_match_kraken_text)
static int kraken_lines(gs_run *run, bool records, int write_all, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_lines) {
    if (!run || !d_out || !n_bytes || !n_lines) return fail(GS_E_INVALID, "NULL argument");
    *d_out = nullptr;
    *n_bytes = *n_lines = 0;
    if (slot < 0 || slot > 1) return fail(GS_E_INVALID, "slot must be 0 or 1");
    TextScan &t = run->text;
    if (t.tickets == 0) return fail(GS_E_STATE, "no text chunk has been submitted");
    if (!records && !t.last_four_line) return fail(GS_E_STATE, "the last chunk was not four-line FASTQ");
    if (records && t.last_four_line) return fail(GS_E_STATE, "the last chunk was four-line FASTQ");
    if (!run->d_tax_off) return fail(GS_E_STATE, "no taxid strings are set (gs_match_set_taxids)");
    const int64_t n = t.last_reads;
    if (n > 0 && !t.d_last_class) return fail(GS_E_STATE, "the last chunk was submitted without a class array");
    HIP_TRY(hipSetDevice(run->db->device));
    uint32_t skip = 0;
    HIP_TRY(hipMemcpyAsync(&skip, t.d_status + (size_t)t.bank * GS_TS_WORDS + GS_TS_SKIP, sizeof(skip), hipMemcpyDeviceToHost, run->stream));
    HIP_TRY(hipStreamSynchronize(run->stream));
    if (skip) return fail(GS_E_STATE, "the last chunk was refused (gs_match_text_status)");
    run->seg_total = 0;
    if (n == 0) return GS_OK;
    run->kr_seg_off.resize((size_t)n + 1);
    run->kr_seg_off[0] = 0;
    int rc = segments_core(run, records ? t.d_fa_seq : t.d_text, (const uint64_t *)t.d_off2, n, records ? 1 : 2, run->kr_seg_off.data());
    if (rc) return rc;
    if (records && (rc = records_heads(t, run->stream))) return rc;
    const size_t n_blocks = ((size_t)n + 255) / 256;
    if ((rc = grow(&run->d_kr_name, &run->kr_name_cap, (size_t)n, run->stream))) return rc;
    if ((rc = grow(&run->d_kr_rec, &run->kr_rec_cap, (size_t)n + 1, run->stream))) return rc;
    if ((rc = grow(&run->d_kr_blocks, &run->kr_blocks_cap, n_blocks + 1, run->stream))) return rc;
    if (!run->d_kr_totals) HIP_TRY(gs_dev_alloc(&run->d_kr_totals, 2 * sizeof(u64)));
    if (!run->h_kr_totals) HIP_TRY(hipHostMalloc((void **)&run->h_kr_totals, 2 * sizeof(u64)));
    GsKrakenParams P{};
    P.text = t.d_text;
    P.nl = t.d_nl;
    if (records) {
        P.rec_line = t.d_rt_line;
        P.off2 = (const unsigned long long *)t.d_off2;
    }
    P.n_reads = n;
    P.k = run->db->info.k;
    P.write_all = write_all != 0;
    P.cls = t.d_last_class;
    P.seg_off = run->d_seg_off;
    P.seg_code = run->d_seg_code;
    P.seg_start = run->d_seg_start;
    P.tax_bytes = run->d_tax_bytes;
    P.tax_off = run->d_tax_off;
    P.name_len = run->d_kr_name;
    P.rec_out = run->d_kr_rec;
    P.rec_block = run->d_kr_blocks;
    P.totals = run->d_kr_totals;
    const bool profile = run->cfg.profile != 0;
    HIP_TRY(hipMemsetAsync(run->d_kr_totals, 0, 2 * sizeof(u64), run->stream));
    if (run->seg_total == 0)  // (no read has a segment: no line; the segment arrays do not exist)
        run->h_kr_totals[0] = run->h_kr_totals[1] = 0;
    else {  // an event pair per pass: the read-back of the total between them is not kernel time
        if ((rc = timer_start(run->kraken_timer, profile, run->stream))) return rc;
        HIP_TRY(gs_launch_kraken_size(&P, run->stream));
        if ((rc = timer_stop(run->kraken_timer, profile, run->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(run->h_kr_totals, run->d_kr_totals, 2 * sizeof(u64), hipMemcpyDeviceToHost, run->stream));
        HIP_TRY(hipStreamSynchronize(run->stream));  // the text's size: the buffer is made for exactly that
    }
    const u64 total = run->h_kr_totals[0];
    if (total > 0) {
        if ((rc = grow(&run->d_kr_out[slot], &run->kr_out_cap[slot], (size_t)total + 16, run->stream))) return rc;
        P.out = run->d_kr_out[slot];
        if ((rc = timer_start(run->kraken_timer, profile, run->stream))) return rc;
        HIP_TRY(gs_launch_kraken_write(&P, run->stream));
        if ((rc = timer_stop(run->kraken_timer, profile, run->stream))) return rc;
    }
    if ((rc = text_touched(t, run->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(run->stream));
    *d_out = total > 0 ? run->d_kr_out[slot] : nullptr;
    *n_bytes = (int64_t)total;
    *n_lines = (int64_t)run->h_kr_totals[1];
    return GS_OK;
}

extern "C" int gs_match_kraken_text(gs_run *run, int write_all, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_lines) try {
    return kraken_lines(run, false, write_all, slot, d_out, n_bytes, n_lines);
}
GS_API_CATCH

extern "C" int gs_match_kraken_records(gs_run *run, int write_all, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_lines) try {
    return kraken_lines(run, true, write_all, slot, d_out, n_bytes, n_lines);
}
GS_API_CATCH

extern "C" int gs_match_kraken_time(gs_run *run, int64_t *launches, double *total_ms) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));
    int rc = timer_collect(run->kraken_timer);
    if (rc) return rc;
    if (launches) *launches = run->kraken_timer.launches;
    if (total_ms) *total_ms = run->kraken_timer.total_ms;
    return GS_OK;
}

extern "C" int gs_match_max_counts(gs_run *run, int16_t *out) {
    if (!run || !out) return fail(GS_E_INVALID, "NULL argument");
    const int N = run->cfg.max_kmer_res_counts;
    if (N <= 0 || !run->d_hit_counts) return fail(GS_E_STATE, "the run was not begun with max_kmer_res_counts > 0");
    if (!run->cfg.count_unique) return fail(GS_E_STATE, "max k-mer counts need count_unique");
    HIP_TRY(hipSetDevice(run->db->device));
    const size_t n_slots = (size_t)run->db->info.n_buckets * GS_SLOTS_PER_BUCKET;
    const size_t nv = (size_t)run->db->info.n_values;
    std::vector<u64> table(n_slots);
    std::vector<uint32_t> counts(n_slots);
    HIP_TRY(hipStreamSynchronize(run->stream));
    // the seen bits: a striped store's and a merged run's are in the run's bitmap (after gs_match_merge: the global one; the table's
    // own bits only know this replica's reads), otherwise in the table
    const bool own_bitmap = run->db->striped() || run->bitmap_merged;
    if (run->db->striped()) {  // the slices of the table from their stripes
        for (int q = 0; q < run->db->n_parts; q++) {
            int64_t tfirst = 0, tlocal = 0;
            const u64 *tq = stripe_table(run->db, q, &tfirst, &tlocal);
            HIP_TRY(hipMemcpy(table.data() + (size_t)tfirst * GS_SLOTS_PER_BUCKET, tq, (size_t)tlocal * GS_SLOTS_PER_BUCKET * sizeof(u64), hipMemcpyDeviceToHost));
        }
    } else
        HIP_TRY(hipMemcpy(table.data(), run->db->d_table, n_slots * sizeof(u64), hipMemcpyDeviceToHost));
    if (own_bitmap) {
        std::vector<uint32_t> tseen((n_slots + 31) / 32);
        HIP_TRY(hipMemcpy(tseen.data(), run->d_bitmap, tseen.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_slots; i++) table[i] = (table[i] & ~1ULL) | ((tseen[i >> 5] >> (i & 31)) & 1u);
    }
    HIP_TRY(hipMemcpy(counts.data(), run->d_hit_counts, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::fill(out, out + (nv + 1) * (size_t)N, (int16_t)0);
    const u64 vmask = ((u64)1 << run->db->dev.vbits) - 1;
    auto update = [N](int16_t count, int16_t *target) {  // updateMaxCounts (:198-209)
        for (int j = 0; j < N; j++)
            if (count > target[j]) {
                for (int kk = N - 1; kk > j; kk--) target[kk] = target[kk - 1];
                target[j] = count;
                return;
            }
    };
    for (size_t i = 0; i < n_slots; i++) {
        const u64 s = table[i];
        if (!(s & 1ULL)) continue;  // bitVector.get(i)
        const int vi = (int)((s >> 1) & vmask) - 1;
        if (vi < 0) continue;
        const int16_t c = (int16_t)(uint16_t)(counts[i] & 0xffffu);  // Java short arithmetic wraps
        update(c, out + (size_t)vi * N);
        update(c, out + nv * (size_t)N);
    }
    if (run->db->n_rec > 0) {  // the k-mers that live in super-k-mer records
        const size_t n_rec = (size_t)run->db->n_rec;
        std::vector<u64> rec(n_rec * GS_REC_WORDS);
        std::vector<uint32_t> rcounts(n_rec * GS_REC_SLOTS);
        std::vector<uint32_t> rseen;  // own_bitmap: the seen bits from the run's bitmap (one word per record bucket)
        const gs_db *db = run->db;
        if (db->striped()) {
            for (int q = 0; q < db->n_parts; q++) {
                const size_t first = (size_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q);
                const size_t local = (size_t)gs_stripe_first(db->dev.rec_bits, (uint32_t)db->n_parts, (uint32_t)q + 1) - first;
                HIP_TRY(hipMemcpy(rec.data() + first * GS_REC_WORDS, db->stripe_base[q], local * GS_REC_WORDS * sizeof(u64), hipMemcpyDeviceToHost));
            }
        } else
            HIP_TRY(hipMemcpy(rec.data(), run->db->d_rec, rec.size() * sizeof(u64), hipMemcpyDeviceToHost));
        if (own_bitmap) {
            rseen.resize(n_rec);
            HIP_TRY(hipMemcpy(rseen.data(), run->d_bitmap + (n_slots + 31) / 32, n_rec * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        HIP_TRY(hipMemcpy(rcounts.data(), run->d_hit_counts + n_slots, rcounts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < n_rec; b++) {
            const u64 *rp = rec.data() + b * GS_REC_WORDS;
            uint32_t seen = (own_bitmap ? rseen[b] : (uint32_t)(rp[0] >> GS_REC_WIN_BITS)) & (uint32_t)(rp[1] >> GS_REC_WIN_BITS);
            for (; seen; seen &= seen - 1) {
                const int j = __builtin_ctz(seen);
                const size_t vi = (size_t)((rp[2 + j / 3] >> (GS_REC_VAL_BITS * (j % 3))) & (GS_REC_MAX_VALUES - 1));
                if (vi >= nv) continue;
                const int16_t c = (int16_t)(uint16_t)(rcounts[b * GS_REC_SLOTS + (size_t)j] & 0xffffu);
                update(c, out + vi * N);
                update(c, out + nv * (size_t)N);
            }
        }
    }
    return GS_OK;
}

// info[0]: 1 if the run's store holds a 15-mer filter; info[1]: |S| (-1: never built); info[2], info[3]: survivors and reads of the
// last submitted batch (survivors -1: that batch went to the match kernel without the prefilter).  Synchronises.
extern "C" int gs_match_prefilter_info(gs_run *run, int64_t *info) {
    if (!run || !info) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));
    info[0] = run->db->d_pf != nullptr ? 1 : 0;
    info[1] = run->db->pf_set;
    info[2] = run->pf_last_survivors;
    info[3] = run->pf_last_reads;
    if (run->pf_last_survivors >= 0) {
        uint32_t n = 0;
        if (run->pf_last_slot >= 0)
            n = run->pf_h[run->pf_last_slot];
        else
            HIP_TRY(hipMemcpy(&n, run->d_long_count + 6, sizeof(n), hipMemcpyDeviceToHost));
        info[2] = (int64_t)n;
    }
    return GS_OK;
}

// info[0]: 1 if the last submitted batch's reads left the match kernel as records (GsSnRec); info[1]: the records of reads of one
// tax id that were booked; info[2]: the reads that left as rows of node codes.  Synchronises.
extern "C" int gs_match_sn_info(gs_run *run, int64_t *info) {
    if (!run || !info) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));
    info[0] = run->sn_last ? 1 : 0;
    info[1] = info[2] = 0;
    if (run->sn_last) {
        uint32_t n[2] = {0, 0};
        HIP_TRY(hipMemcpy(n, run->d_long_count + 7, sizeof(n), hipMemcpyDeviceToHost));
        info[1] = (int64_t)n[0];
        info[2] = (int64_t)n[1];
    }
    return GS_OK;
}

// *gateless: 1 if the last submitted batch went through the FIXED loop without the minimizer gate; *predicted_pass: the probability
// the gate rule used for it (-1: the batch could not take that loop, nothing was asked).  Host state only: does not synchronise.
extern "C" int gs_match_gate_info(gs_run *run, int *gateless, double *predicted_pass) {
    if (!run || !gateless || !predicted_pass) return fail(GS_E_INVALID, "NULL argument");
    *gateless = run->gate_last_gateless ? 1 : 0;
    *predicted_pass = run->gate_last_pass;
    return GS_OK;
}

extern "C" int gs_match_kernel_time(gs_run *run, int64_t *launches, double *total_ms) {
    if (!run) return fail(GS_E_INVALID, "run is NULL");
    HIP_TRY(hipSetDevice(run->db->device));
    HIP_TRY(hipStreamSynchronize(run->stream));
    int rc = timer_collect(run->timer);
    if (rc) return rc;
    if (launches) *launches = run->timer.launches;
    if (total_ms) *total_ms = run->timer.total_ms;
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------
struct gs_bloom {
    int device = 0;
    int kind = 0;
    int64_t bits = 0;
    int32_t n_hashes = 0;
    int64_t n_words = 0;
    int32_t k = 0;                                        // what gs_bloom_get_info reports beyond the geometry: 0 / -1 / 0 = unknown
    int64_t expected_insertions = -1, n_inserted = -1;
    double fpp = 0.0;
    u64 *d_words = nullptr;
    int64_t *d_factors = nullptr;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    HostStage host{false};  // host batches (GS_MEM_HOST); d_flags is accept, d_class stays empty
    TextScan text;   // text mode (gs_filter_submit_text)
    KernelTimer timer;
};

extern "C" int gs_bloom_create(gs_bloom **out, int device, int kind, int64_t bits, int32_t n_hashes,
                               const int64_t *hash_factors, const uint64_t *words, int64_t n_words) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (kind < GS_BLOOM_XOR || kind > GS_BLOOM_BLOCKED) return fail(GS_E_INVALID, "unknown bloom kind");
    if (bits < 1 || !hash_factors || !words || n_words < 1) return fail(GS_E_INVALID, "bad bloom arrays");
    if (kind != GS_BLOOM_BLOCKED) {
        if (n_hashes < 1 || n_hashes > 64) return fail(GS_E_INVALID, "n_hashes must be in [1,64]");
        if (n_words < (bits + 63) / 64) return fail(GS_E_INVALID, "words shorter than bits");
        if (bits > ((int64_t)1 << 37)) return fail(GS_E_UNSUPPORTED, "filters above 2^37 bits (16 GiB) are not supported");
    } else {
        n_hashes = 1;
        if (n_words < bits + 17) return fail(GS_E_INVALID, "blocked filter needs buckets+17 words");
    }
    int rc = use_device(device);
    if (rc) return rc;
    gs_bloom *b = new gs_bloom();
    b->device = device;
    b->kind = kind;
    b->bits = bits;
    b->n_hashes = n_hashes;
    b->n_words = n_words;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) b->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&b->d_words, sizeof(u64) * (size_t)n_words);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&b->d_factors, sizeof(int64_t) * (size_t)n_hashes);
    if (e == hipSuccess) e = hipMemcpy(b->d_words, words, sizeof(u64) * (size_t)n_words, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_factors, hash_factors, sizeof(int64_t) * (size_t)n_hashes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        gs_bloom_destroy(b);
        return hip_fail(e, "bloom upload");
    }
    *out = b;
    return GS_OK;
}
GS_API_CATCH

// java.util.Random (the hash factors of the reference's filters are its first nextLong() values for seed 42,
// C/bloom/AbstractKMerBloomFilter.java:78,105-109)
struct JavaRandom {
    uint64_t s;
    explicit JavaRandom(int64_t seed) : s(((uint64_t)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int32_t next(int bits) {
        s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)(int64_t)(s >> (48 - bits));
    }
    int64_t next_long() {
        const int64_t hi = (int64_t)next(32), lo = (int64_t)next(32);
        return (int64_t)(((uint64_t)hi << 32) + (uint64_t)lo);
    }
};

extern "C" int gs_bloom_build(gs_bloom **out, int device, int kind, const int64_t *kmers, int64_t n_kmers, int mem, int64_t expected_insertions,
                              double fpp) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (kind != GS_BLOOM_XOR && kind != GS_BLOOM_MURMUR)
        return fail(GS_E_UNSUPPORTED, "gs_bloom_build makes XOR and Murmur filters (the reference's index filters); blocked filters: gs_bloom_create");
    if (n_kmers < 0 || (n_kmers > 0 && !kmers) || expected_insertions < 1 || !(fpp > 0.0 && fpp < 1.0)) return fail(GS_E_INVALID, "bad argument");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    // AbstractKMerBloomFilter.optimalNumOfBits :183-185, optimalNumOfHashFunctions :172-174 (Java double arithmetic)
    const double dbits = -(double)expected_insertions * std::log(fpp) / (std::log(2.0) * std::log(2.0));
    int64_t bits = (int64_t)dbits;
    if (bits < 1) bits = 1;
    if (bits > ((int64_t)1 << 37)) return fail(GS_E_UNSUPPORTED, "filters above 2^37 bits (16 GiB) are not supported");
    int64_t nh = (int64_t)std::floor((double)bits / (double)expected_insertions * std::log(2.0) + 0.5);  // Math.round
    if (nh < 1) nh = 1;
    if (nh > 64) return fail(GS_E_UNSUPPORTED, "more than 64 hash functions");
    std::vector<int64_t> factors((size_t)nh);
    JavaRandom rnd(42);
    for (int64_t i = 0; i < nh; i++) factors[(size_t)i] = rnd.next_long();
    int rc = use_device(device);
    if (rc) return rc;
    gs_bloom *b = new gs_bloom();
    b->device = device;
    b->kind = kind;
    b->bits = bits;
    b->n_hashes = (int32_t)nh;
    b->n_words = (bits + 63) / 64;
    b->expected_insertions = expected_insertions;
    b->n_inserted = n_kmers;
    b->fpp = fpp;
    hipDeviceProp_t prop;
    int64_t *d_keys = nullptr;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) b->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&b->d_words, sizeof(u64) * (size_t)b->n_words);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&b->d_factors, sizeof(int64_t) * (size_t)nh);
    if (e == hipSuccess) e = hipMemsetAsync(b->d_words, 0, sizeof(u64) * (size_t)b->n_words, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_factors, factors.data(), sizeof(int64_t) * (size_t)nh, hipMemcpyHostToDevice, b->stream);
    const int64_t *keys = kmers;
    if (e == hipSuccess && mem == GS_MEM_HOST && n_kmers > 0) {
        e = gs_dev_alloc((void **)&d_keys, sizeof(int64_t) * (size_t)n_kmers);
        if (e == hipSuccess) e = hipMemcpyAsync(d_keys, kmers, sizeof(int64_t) * (size_t)n_kmers, hipMemcpyHostToDevice, b->stream);
        keys = d_keys;
    }
    if (e == hipSuccess) e = gs_launch_bloom_xor_put(keys, n_kmers, bits, b->d_factors, (int)nh, kind == GS_BLOOM_MURMUR, b->d_words, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    gs_dev_free(d_keys);
    if (e != hipSuccess) {
        gs_bloom_destroy(b);
        return hip_fail(e, "gs_bloom_build");
    }
    *out = b;
    return GS_OK;
}
GS_API_CATCH

// ensureExpectedSize(n, false) of the three filter kinds, n >= 0 (AbstractKMerBloomFilter.java:96-113,172-185;
// BlockedKMerBloomFilter: 10 bits per key); the limits are those of gs_bloom_create / gs_bloom_build
static int bloom_geometry(int kind, int64_t n, double fpp, int64_t &bits, int64_t &nh, int64_t &n_words) {
    if (kind == GS_BLOOM_BLOCKED) {
        const int64_t entries = n < 1 ? 1 : n;
        if (entries > ((int64_t)1 << 40)) return fail(GS_E_UNSUPPORTED, "blocked filters above 2^40 keys are not supported");
        bits = (entries * 10 + 63) / 64;
        nh = 1;
        n_words = bits + 17;
        return GS_OK;
    }
    if (n == 0) {  // (Math.round(+Inf) cast to int is -1, max(1, -1) = 1)
        bits = nh = n_words = 1;
        return GS_OK;
    }
    const double dbits = -(double)n * std::log(fpp) / (std::log(2.0) * std::log(2.0));
    if (!(dbits < 1.0e18)) return fail(GS_E_UNSUPPORTED, "filters above 2^37 bits (16 GiB) are not supported");
    bits = (int64_t)dbits;
    if (bits < 1) bits = 1;
    if (bits > ((int64_t)1 << 37)) return fail(GS_E_UNSUPPORTED, "filters above 2^37 bits (16 GiB) are not supported");
    nh = (int64_t)std::floor((double)bits / (double)n * std::log(2.0) + 0.5);  // Math.round
    if (nh < 1) nh = 1;
    if (nh > 64) return fail(GS_E_UNSUPPORTED, "more than 64 hash functions");
    n_words = (bits + 63) / 64;
    return GS_OK;
}

// The index goal on a device store (gs_index.hip): a count pass of the walk sizes the filter, the put pass fills it and counts
// again.  Beyond the store and the filter the call holds the requested bitmap (n_values bits) and two counters.
extern "C" int gs_bloom_build_db(gs_bloom **out, gs_db *db, int kind, const uint8_t *requested, int64_t expected_insertions, double fpp,
                                 int64_t *n_inserted) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (kind < GS_BLOOM_XOR || kind > GS_BLOOM_BLOCKED) return fail(GS_E_INVALID, "unknown bloom kind");
    if (expected_insertions == 0) return fail(GS_E_INVALID, "expected_insertions must be >= 1, or negative for the count");
    if (kind != GS_BLOOM_BLOCKED && !(fpp > 0.0 && fpp < 1.0)) return fail(GS_E_INVALID, "fpp must be in (0, 1)");
    if (!db) return fail(GS_E_INVALID, "db is NULL");
    if (!requested) return fail(GS_E_INVALID, "requested is NULL");
    if (db->striped()) return fail(GS_E_UNSUPPORTED, "gs_bloom_build_db: a stripe holds a share of the k-mers; build the index from the whole store");
    const int32_t nv = db->info.n_values;
    std::vector<uint32_t> bitmap(((size_t)nv + 31) / 32, 0u);
    for (int32_t v = 0; v < nv; v++)
        if (requested[v]) bitmap[(size_t)v >> 5] |= 1u << (v & 31);
    HIP_TRY(hipSetDevice(db->device));
    gs_bloom *b = new gs_bloom();
    b->device = db->device;
    b->kind = kind;
    b->k = db->info.k;
    b->n_cu = db->n_cu;
    const GsExportParams S = export_params(db, -1, 0);
    GsIndexParams P{};
    P.rec = S.rec;
    P.n_rec = S.n_rec;
    P.tab = S.tab;
    P.tab_first = S.tab_first;
    P.n_tab = S.n_tab;
    P.bucket_bits = S.bucket_bits;
    P.vbits = S.vbits;
    P.k = S.k;
    P.n_values = nv;
    P.kind = kind;
    uint32_t *d_bitmap = nullptr;
    u64 *d_count = nullptr;  // [0]: the count pass, [1]: the put pass
    u64 counts[2] = {0, 0};
    HipSteps step{"gs_bloom_build_db"};
    int rc = GS_OK;
    int64_t bits = 0, nh = 0;
    // GS_INDEX_TRACE=1: the two passes between events, on stderr (developer aid, tools/index_build_rate.py)
    const bool trace = getenv("GS_INDEX_TRACE") != nullptr && atoi(getenv("GS_INDEX_TRACE")) != 0;
    KernelTimer t_count, t_put;
    std::vector<int64_t> factors;  // (read by an asynchronous copy: lives until the handle's stream has been drained)
    bool ok = step(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking), "stream") &&
              step(gs_dev_alloc((void **)&d_bitmap, sizeof(uint32_t) * bitmap.size()), "bitmap") &&
              step(gs_dev_alloc((void **)&d_count, sizeof(counts)), "counters") &&
              step(hipMemsetAsync(d_count, 0, sizeof(counts), b->stream), "counters") &&
              step(hipMemcpyAsync(d_bitmap, bitmap.data(), sizeof(uint32_t) * bitmap.size(), hipMemcpyHostToDevice, b->stream), "bitmap");
    if (ok) {
        P.requested = d_bitmap;
        P.count = d_count;
        ok = timer_start(t_count, trace, b->stream) == GS_OK && step(gs_launch_index(&P, db->n_cu, b->stream), "count pass") &&
             timer_stop(t_count, trace, b->stream) == GS_OK && step(hipMemcpyAsync(&counts[0], d_count, sizeof(u64), hipMemcpyDeviceToHost, b->stream), "count") &&
             step(hipStreamSynchronize(b->stream), "count pass");
    }
    if (ok) {
        b->n_inserted = (int64_t)counts[0];
        b->expected_insertions = expected_insertions < 0 ? b->n_inserted : expected_insertions;
        b->fpp = kind == GS_BLOOM_BLOCKED ? 0.0 : fpp;
        rc = bloom_geometry(kind, b->expected_insertions, fpp, bits, nh, b->n_words);
        ok = rc == GS_OK;
    }
    if (ok) {
        b->bits = bits;
        b->n_hashes = (int32_t)nh;
        factors.resize((size_t)nh);
        JavaRandom rnd(42);
        for (int64_t i = 0; i < nh; i++) factors[(size_t)i] = rnd.next_long();
        uint64_t mg = 0;
        int sh = 0;
        gs_magic_u64((u64)bits, mg, sh);  // gs_absmod.h
        ok = step(gs_dev_alloc((void **)&b->d_words, sizeof(u64) * (size_t)b->n_words), "filter words") &&
             step(gs_dev_alloc((void **)&b->d_factors, sizeof(int64_t) * (size_t)nh), "hash factors") &&
             step(hipMemsetAsync(b->d_words, 0, sizeof(u64) * (size_t)b->n_words, b->stream), "filter words") &&
             step(hipMemcpyAsync(b->d_factors, factors.data(), sizeof(int64_t) * (size_t)nh, hipMemcpyHostToDevice, b->stream), "hash factors");
        P.put = 1;
        P.n_hashes = (int32_t)nh;
        P.hash_inv = nh >= 2 ? (uint32_t)((((uint64_t)1 << 32) + (uint64_t)nh - 1) / (uint64_t)nh) : 0u;
        P.bits = (u64)bits;
        P.magic = mg;
        P.magic_shift = sh;
        P.factors = b->d_factors;
        P.words = b->d_words;
        P.count = d_count + 1;
        ok = ok && timer_start(t_put, trace, b->stream) == GS_OK &&
             (counts[0] == 0 || step(gs_launch_index(&P, db->n_cu, b->stream), "put pass")) && timer_stop(t_put, trace, b->stream) == GS_OK &&
             step(hipMemcpyAsync(&counts[1], d_count + 1, sizeof(u64), hipMemcpyDeviceToHost, b->stream), "count") &&
             step(hipStreamSynchronize(b->stream), "put pass");
    }
    if (!ok && b->stream) hipStreamSynchronize(b->stream);
    if (ok && trace && timer_collect(t_count) == GS_OK && timer_collect(t_put) == GS_OK)
        fprintf(stderr, "[gs_bloom_build_db] kind %d, %lld k-mers, %lld hashes: count pass %.3f ms, put pass %.3f ms\n", kind, (long long)counts[0],
                (long long)nh, t_count.total_ms, t_put.total_ms);
    timer_free(t_count);
    timer_free(t_put);
    gs_dev_free(d_bitmap);
    gs_dev_free(d_count);
    if (ok && counts[1] != counts[0])
        rc = fail(GS_E_HIP, "gs_bloom_build_db: the put pass inserted " + std::to_string(counts[1]) + " k-mers, the count pass found " +
                                std::to_string(counts[0]));
    else if (!ok && rc == GS_OK)
        rc = step.rc ? step.rc : GS_E_HIP;  // (a trace event that could not be made: its message stands)
    if (rc) {
        gs_bloom_destroy(b);
        return rc;
    }
    if (n_inserted) *n_inserted = b->n_inserted;
    *out = b;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_bloom_get_info(gs_bloom *b, gs_bloom_info *info) {
    if (!b || !info) return fail(GS_E_INVALID, "NULL argument");
    *info = gs_bloom_info{};
    info->kind = b->kind;
    info->k = b->k;
    info->n_hashes = b->n_hashes;
    info->bits = b->bits;
    info->n_words = b->n_words;
    info->expected_insertions = b->expected_insertions;
    info->n_inserted = b->n_inserted;
    info->fpp = b->fpp;
    return GS_OK;
}

// ---- native index file (include/gsgpu.h): the header, its checks and the reader are host code of their own (gs_indexfile.h)
extern "C" int gs_bloom_save(gs_bloom *b, const char *path) try {
    if (!b || !path) return fail(GS_E_INVALID, "NULL argument");
    GsIndexFileHeader h{};
    memcpy(h.magic, "GSINDEX1", 8);
    h.kind = b->kind;
    h.k = b->k;
    h.n_hashes = b->n_hashes;
    h.bits = b->bits;
    h.n_words = b->kind == GS_BLOOM_BLOCKED ? b->bits + 17 : (b->bits + 63) / 64;  // (gs_bloom_create takes longer arrays: the file holds the filter's own)
    h.expected_insertions = b->expected_insertions;
    h.n_inserted = b->n_inserted;
    h.fpp = b->fpp;
    if (const char *why = gs_index_header_defect(h)) return fail(GS_E_UNSUPPORTED, std::string("gs_bloom_save: ") + why);
    std::vector<int64_t> factors((size_t)b->n_hashes);
    std::vector<u64> words((size_t)h.n_words);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(factors.data(), b->d_factors, factors.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(words.data(), b->d_words, words.size() * sizeof(u64), hipMemcpyDeviceToHost));
    h.checksum = gs_index_checksum(factors, words);
    FILE *f = fopen(path, "wb");
    if (!f) return fail(GS_E_IO, std::string("cannot open ") + path);
    bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && fwrite(factors.data(), sizeof(int64_t), factors.size(), f) == factors.size() &&
              fwrite(words.data(), sizeof(u64), words.size(), f) == words.size();
    ok = (fclose(f) == 0) && ok;
    return ok ? GS_OK : fail(GS_E_IO, std::string("short write to ") + path);
}
GS_API_CATCH

extern "C" int gs_bloom_load(gs_bloom **out, int device, const char *path) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!path) return fail(GS_E_INVALID, "path is NULL");
    GsIndexFileHeader h{};
    std::vector<int64_t> factors;
    std::vector<u64> words;
    std::string why;
    const int got = gs_index_file_read(path, h, factors, words, why);  // every check of the file, before a device is touched
    if (got != GS_INDEXFILE_OK) return fail(got == GS_INDEXFILE_IO ? GS_E_IO : GS_E_INVALID, why);
    gs_bloom *b = nullptr;
    const int rc = gs_bloom_create(&b, device, h.kind, h.bits, h.n_hashes, factors.data(), (const uint64_t *)words.data(), h.n_words);
    if (rc) return rc;
    b->k = h.k;
    b->expected_insertions = h.expected_insertions;
    b->n_inserted = h.n_inserted;
    b->fpp = h.fpp;
    *out = b;
    return GS_OK;
}
GS_API_CATCH

// geometry and contents of a filter (tests, and hosts that keep the filter in the reference's own object): words may be NULL
extern "C" int gs_bloom_get(gs_bloom *b, int64_t *bits, int32_t *n_hashes, int64_t *hash_factors, uint64_t *words, int64_t n_words) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    if (bits) *bits = b->bits;
    if (n_hashes) *n_hashes = b->n_hashes;
    if (hash_factors) HIP_TRY(hipMemcpy(hash_factors, b->d_factors, sizeof(int64_t) * (size_t)b->n_hashes, hipMemcpyDeviceToHost));
    if (words) {
        if (n_words < b->n_words) return fail(GS_E_INVALID, "words is shorter than the filter");
        HIP_TRY(hipMemcpy(words, b->d_words, sizeof(u64) * (size_t)b->n_words, hipMemcpyDeviceToHost));
    }
    return GS_OK;
}

extern "C" int gs_bloom_destroy(gs_bloom *b) {
    if (!b) return GS_OK;
    hipSetDevice(b->device);
    if (b->stream) hipStreamSynchronize(b->stream);
    timer_free(b->timer);
    gs_dev_free(b->d_words);
    gs_dev_free(b->d_factors);
    stage_free(b->host);
    text_free(b->text);
    if (b->stream) hipStreamDestroy(b->stream);
    delete b;
    return GS_OK;
}

static int filter_launch(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *d_seq,
                         const uint64_t *d_off, int64_t n_reads, uint8_t *d_acc, int off_stride, const uint32_t *d_skip,
                         int profile) {
    GsFilterParams P{};
    P.kind = b->kind;
    P.k = k;
    P.min_pos_count = min_pos_count;
    P.positive_ratio = positive_ratio;
    P.bits = (u64)b->bits;
    P.n_hashes = b->n_hashes;
    P.words = b->d_words;
    P.factors = b->d_factors;
    {
        uint64_t mg = 0;
        int sh = 0;
        gs_magic_u64((u64)b->bits, mg, sh);  // gs_absmod.h
        P.magic = mg;
        P.magic_shift = sh;
    }
    P.seq = d_seq;
    P.off = d_off;
    P.n_reads = n_reads;
    P.accept = d_acc;
    P.off_stride = off_stride;
    P.skip = d_skip;
    int occ = gs_filter_occupancy();
    if (occ < 1) occ = 1;
    if (const char *ev = getenv("GS_FILTER_BLOCKS_PER_CU")) {
        const int v = atoi(ev);
        if (v >= 1 && v <= 16) occ = v;
    }
    int grid = (int)std::min<int64_t>((int64_t)b->n_cu * occ, (n_reads + 3) / 4);
    if (grid < 1) grid = 1;
    const int rc = timer_start(b->timer, profile != 0, b->stream);
    if (rc) return rc;
    HIP_TRY(gs_launch_filter(&P, grid, b->stream));
    return timer_stop(b->timer, profile != 0, b->stream);
}

extern "C" int gs_filter_submit(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *seq,
                                const uint64_t *offsets, int64_t n_reads, int mem, uint8_t *accept, int profile) try {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (n_reads < 0 || (n_reads > 0 && (!seq || !offsets || !accept))) return fail(GS_E_INVALID, "bad batch arrays");
    if (n_reads == 0) return GS_OK;
    HIP_TRY(hipSetDevice(b->device));
    if (mem == GS_MEM_DEVICE) return filter_launch(b, k, min_pos_count, positive_ratio, seq, offsets, n_reads, accept, 1, nullptr, profile);
    if (mem != GS_MEM_HOST) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HostStage &h = b->host;
    int rc = stage_room(h, (size_t)(offsets[n_reads] - offsets[0]), (size_t)n_reads, b->stream);
    if (!rc) rc = stage_upload(h, seq, offsets, n_reads, b->stream);
    if (!rc) rc = filter_launch(b, k, min_pos_count, positive_ratio, h.d_seq, h.d_off, n_reads, h.d_flags, 1, nullptr, profile);
    if (!rc) rc = stage_download(h, nullptr, accept, n_reads, b->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
    return timer_collect(b->timer);
}
GS_API_CATCH

extern "C" int gs_filter_sync(gs_bloom *b) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return timer_collect(b->timer);
}

// ---- text mode of the filter (see gs_match_submit_text) ----
static int filter_submit_text(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *text, int64_t n_bytes,
                              int64_t n_lines, int mem, uint8_t *accept, uint32_t *newlines, int profile, int64_t *ticket,
                              int64_t fasta_records, int64_t *ml_out) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (n_lines > 0 && !accept) return fail(GS_E_INVALID, "accept is NULL");
    HIP_TRY(hipSetDevice(b->device));
    TextBatch tb;
    int rc = text_batch(b->text, b->stream, text, n_bytes, n_lines, mem, k, ticket, fasta_records, ml_out, &tb);
    if (rc || tb.n_reads == 0) return rc;
    HostStage &h = b->host;
    if (!tb.dev_out && (rc = stage_room_reads(h, (size_t)tb.n_reads, b->stream))) return rc;
    uint8_t *d_acc = tb.dev_out ? accept : h.d_flags;
    // a refused chunk leaves `accept` untouched: zero it so that stale flags never look like results
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)tb.n_reads, b->stream));
    rc = filter_launch(b, k, min_pos_count, positive_ratio, tb.d_seq, (const uint64_t *)b->text.d_off2, tb.n_reads, d_acc, tb.off_stride, tb.d_skip, profile);
    if (rc) return rc;
    if ((rc = text_touched(b->text, b->stream))) return rc;
    b->text.d_last_flags = d_acc;
    if (!tb.dev_out && (rc = stage_download(h, nullptr, accept, tb.n_reads, b->stream))) return rc;
    if (newlines)
        HIP_TRY(hipMemcpyAsync(newlines, b->text.d_nl, sizeof(uint32_t) * (size_t)n_lines, tb.dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, b->stream));
    return GS_OK;
}

extern "C" int gs_filter_submit_text(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                                     int64_t n_bytes, int64_t n_lines, int mem, uint8_t *accept, uint32_t *newlines,
                                     int profile, int64_t *ticket) try {
    return filter_submit_text(b, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, mem, accept, newlines, profile, ticket, -1, nullptr);
}
GS_API_CATCH

extern "C" int gs_filter_submit_fasta(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                                      int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem, uint8_t *accept,
                                      uint32_t *newlines, int64_t *ticket) try {
    if (n_records < 0) return fail(GS_E_INVALID, "n_records < 0");
    return filter_submit_text(b, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, mem, accept, newlines, 0, ticket, n_records, nullptr);
}
GS_API_CATCH

extern "C" int gs_filter_submit_fastq_ml(gs_bloom *b, int k, int min_pos_count, double positive_ratio, const uint8_t *text,
                                         int64_t n_bytes, int64_t n_lines, int mem, uint8_t *accept, uint32_t *newlines,
                                         int64_t *n_records, int64_t *consumed_bytes, int64_t *consumed_lines, int64_t *ticket) try {
    if (!n_records || !consumed_bytes) return fail(GS_E_INVALID, "NULL argument");
    int64_t out[3] = {0, 0, 0};
    const int rc = filter_submit_text(b, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, mem, accept, newlines, 0, ticket, -1, out);
    return ml_report(rc, out, n_records, consumed_bytes, consumed_lines);
}
GS_API_CATCH

// nextEntry's rewriteInput on the device (FastqBloomFilter.java:92-105): the accepted (which != 0) or the other records of the last chunk
extern "C" int gs_filter_compact_text(gs_bloom *b, int which, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    return text_compact(b->text, b->stream, 0xff, which != 0, which != 0, slot, with_probs, d_out, n_bytes, n_records);
}

// the same for the records of a FASTA or general FASTQ chunk (gs_rewrite.hip)
extern "C" int gs_filter_compact_records(gs_bloom *b, int which, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) try {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    return text_records(b->text, b->stream, b->n_cu, 0xff, which != 0, which != 0, with_probs, slot, nullptr, false, d_out, n_bytes, n_records);
}
GS_API_CATCH

extern "C" int gs_filter_text_read_bounds(gs_bloom *b, uint64_t *bounds) {
    if (!b || !bounds) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    const int rc = text_read_bounds(b->text, b->stream, bounds, "the last chunk was four-line FASTQ: its reads lie in the text (newlines)");
    return rc ? rc : timer_collect(b->timer);
}

extern "C" int gs_filter_text_line_classes(gs_bloom *b, uint8_t *classes) {
    if (!b || !classes) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    const int rc = text_line_classes(b->text, b->stream, classes);
    return rc ? rc : timer_collect(b->timer);
}

extern "C" int gs_filter_get_device(gs_bloom *b, int *device) {
    if (!b || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = b->device;
    return GS_OK;
}

extern "C" int gs_filter_text_wait_copy(gs_bloom *b, int64_t ticket) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    return text_wait_copy(b->text, ticket);
}

extern "C" int gs_filter_text_status(gs_bloom *b, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    int rc = text_status(b->text, b->stream, failed_ticket, first_bad_record, totals);
    if (rc) return rc;
    return timer_collect(b->timer);
}

extern "C" int gs_filter_text_reset(gs_bloom *b, int clear_totals) {
    if (!b) return fail(GS_E_INVALID, "bloom is NULL");
    HIP_TRY(hipSetDevice(b->device));
    return text_reset(b->text, clear_totals != 0, b->stream);
}

extern "C" int gs_filter_kernel_time(gs_bloom *b, int64_t *launches, double *total_ms) {
    int rc = gs_filter_sync(b);
    if (rc) return rc;
    if (launches) *launches = b->timer.launches;
    if (total_ms) *total_ms = b->timer.total_ms;
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// reads: the text stage without a store or a filter -- extract and fasta2fastq (gs_rewrite.hip)
// ---------------------------------------------------------------------------------------------------
struct gs_reads {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    TextScan text;
    uint8_t *d_accept = nullptr, *d_key = nullptr;  // the flags of a chunk whose caller wants them in host memory; the key
    size_t accept_cap = 0, key_cap = 0;
    std::string key;  // what d_key holds: the caller's key is copied here first, so its memory is free again when a select call returns
    uint32_t *d_rec_line = nullptr, *d_piece = nullptr;
    u64 *d_rec_out = nullptr, *d_rec_block = nullptr;
    size_t rec_line_cap = 0, piece_cap = 0, rec_out_cap = 0, rec_block_cap = 0;
    u64 *d_tot = nullptr, *h_tot = nullptr;  // GsRewriteParams::totals and their page-locked landing area
    uint8_t *d_out[2] = {nullptr, nullptr};  // the FASTA -> FASTQ text, two slots
    size_t out_cap[2] = {0, 0};
    const uint8_t *d_last_accept = nullptr;  // where the flags of the last chunk, a FASTA one, lie on the device
    bool last_ml = false;
    bool last_select = false;  // the last chunk came through a select call that took it (a chunk of 0 records included)
    bool profile = false;  // gs_reads_kernel_time: the FASTA -> FASTQ text kernels (sizes, offsets, copy) between events
    KernelTimer timer;
    KernelTimer select_timer, gather_timer;  // gs_reads_phase_times: a chunk from its submission to its flags; the four-line gather
};

extern "C" int gs_reads_destroy(gs_reads *h) {
    if (!h) return GS_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    timer_free(h->timer);
    timer_free(h->select_timer);
    timer_free(h->gather_timer);
    text_free(h->text);
    gs_dev_free(h->d_accept);
    gs_dev_free(h->d_key);
    gs_dev_free(h->d_rec_line);
    gs_dev_free(h->d_piece);
    gs_dev_free(h->d_rec_out);
    gs_dev_free(h->d_rec_block);
    gs_dev_free(h->d_tot);
    if (h->h_tot) hipHostFree(h->h_tot);
    gs_dev_free(h->d_out[0]);
    gs_dev_free(h->d_out[1]);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return GS_OK;
}

extern "C" int gs_reads_create(gs_reads **out, int device) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    int rc = use_device(device);
    if (rc) return rc;
    gs_reads *h = new gs_reads();
    h->device = device;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc((void **)&h->d_tot, sizeof(u64) * 4);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_tot, sizeof(u64) * 4);
    if (e != hipSuccess) {
        gs_reads_destroy(h);
        return hip_fail(e, "gs_reads_create");
    }
    *out = h;
    return GS_OK;
}
GS_API_CATCH

// what the rewrite kernels take from the text stage's latest chunk (ReadEntry mode; text_submit fills the same fields in goal mode)
static void reads_params(gs_reads *h, GsRewriteParams *R) {
    TextScan &t = h->text;
    R->text = t.d_text;
    R->n_lines = t.last_lines;
    R->n_records = t.last_reads;
    R->nl = t.d_nl;
    R->fa_scan = (unsigned long long *)t.d_fa_scan;
    R->fa_block = (unsigned long long *)t.d_fa_block;
    R->line_dst = t.d_line_dst;
    R->fa_seq = t.d_fa_seq;
    R->off2 = (unsigned long long *)t.d_off2;
    R->status = t.d_status + (size_t)t.bank * GS_TS_WORDS;
    R->gate = R->status + GS_TS_SKIP;
    R->rec_line = h->d_rec_line;
    R->rec_out = (unsigned long long *)h->d_rec_out;
    R->rec_block = (unsigned long long *)h->d_rec_block;
    R->piece_rec = h->d_piece;
    R->totals = (unsigned long long *)h->d_tot;
}

// room for the per-record arrays of n_records records and for `bound` bytes of text in slot `slot` (slot < 0: none)
static int reads_room(gs_reads *h, int64_t n_records, int slot, size_t bound) {
    int rc;
    if ((rc = grow(&h->d_rec_line, &h->rec_line_cap, (size_t)n_records + 1, h->stream))) return rc;
    if (slot < 0) return GS_OK;
    if ((rc = grow(&h->d_rec_out, &h->rec_out_cap, (size_t)n_records + 1, h->stream))) return rc;
    if ((rc = grow(&h->d_rec_block, &h->rec_block_cap, (size_t)n_records / 256 + 2, h->stream))) return rc;
    if ((rc = grow(&h->d_piece, &h->piece_cap, bound / 4096 + 2, h->stream))) return rc;
    return grow(&h->d_out[slot], &h->out_cap[slot], bound, h->stream);
}

static int reads_select(gs_reads *h, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, const uint8_t *key, int32_t key_len,
                        uint8_t *accept, uint32_t *newlines, int64_t *ticket, int64_t fasta_records, int64_t *ml_out) {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    if (k < 1 || k > 31) return fail(GS_E_INVALID, "k must be in [1,31]");
    if (!key || key_len < 1) return fail(GS_E_INVALID, "the key is empty");
    for (int32_t i = 0; i < key_len; i++)  // (Java compares byte != char: a byte >= 0x80 never matches; a NUL ends the descriptor)
        if (key[i] == 0 || key[i] >= 0x80) return fail(GS_E_INVALID, "the key holds a NUL byte or a byte >= 0x80");
    if (n_lines > 0 && !accept) return fail(GS_E_INVALID, "accept is NULL");
    HIP_TRY(hipSetDevice(h->device));
    TextScan &t = h->text;
    TextBatch tb;
    int rc = timer_start(h->select_timer, h->profile, h->stream);
    if (rc) return rc;
    rc = text_batch(t, h->stream, text, n_bytes, n_lines, mem, k, ticket, fasta_records, ml_out, &tb);
    h->d_last_accept = nullptr;
    h->last_ml = ml_out != nullptr;
    h->last_select = rc == GS_OK;
    if (rc || tb.n_reads == 0) return rc;
    if (!h->d_key || h->key.size() != (size_t)key_len || memcmp(h->key.data(), key, (size_t)key_len) != 0) {
        if ((rc = grow(&h->d_key, &h->key_cap, (size_t)key_len, h->stream))) return rc;
        h->key.assign((const char *)key, (size_t)key_len);
        HIP_TRY(hipMemcpyAsync(h->d_key, h->key.data(), (size_t)key_len, hipMemcpyHostToDevice, h->stream));
    }
    if (!tb.dev_out && (rc = grow(&h->d_accept, &h->accept_cap, (size_t)tb.n_reads, h->stream))) return rc;
    uint8_t *d_acc = tb.dev_out ? accept : h->d_accept;
    // a refused chunk leaves `accept` untouched: zero it so that stale flags never look like results
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)tb.n_reads, h->stream));
    if (tb.fasta) {  // the descriptor line of every record
        if ((rc = reads_room(h, tb.n_reads, -1, 0))) return rc;
        GsRewriteParams R{};
        reads_params(h, &R);
        R.n_records = tb.n_reads;
        R.line_class = ml_out ? t.d_ml_class : nullptr;
        HIP_TRY(gs_launch_rewrite_heads(&R, h->stream));
    }
    HIP_TRY(gs_launch_select(t.d_text, t.d_nl, tb.fasta ? h->d_rec_line : nullptr, tb.n_reads, h->d_key, key_len, tb.d_skip, d_acc, h->stream));
    if ((rc = timer_stop(h->select_timer, h->profile, h->stream))) return rc;
    if ((rc = text_touched(t, h->stream))) return rc;
    t.d_last_flags = d_acc;
    if (tb.fasta && !ml_out) h->d_last_accept = d_acc;
    if (!tb.dev_out) HIP_TRY(hipMemcpyAsync(accept, d_acc, (size_t)tb.n_reads, hipMemcpyDeviceToHost, h->stream));
    if (newlines)
        HIP_TRY(hipMemcpyAsync(newlines, t.d_nl, sizeof(uint32_t) * (size_t)t.last_lines, tb.dev_out ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return GS_OK;
}

extern "C" int gs_reads_select_text(gs_reads *h, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, const uint8_t *key, int32_t key_len,
                                    uint8_t *accept, uint32_t *newlines, int64_t *ticket) try {
    return reads_select(h, k, text, n_bytes, n_lines, mem, key, key_len, accept, newlines, ticket, -1, nullptr);
}
GS_API_CATCH

extern "C" int gs_reads_select_fasta(gs_reads *h, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem,
                                     const uint8_t *key, int32_t key_len, uint8_t *accept, uint32_t *newlines, int64_t *ticket) try {
    if (n_records < 0) return fail(GS_E_INVALID, "n_records < 0");
    return reads_select(h, k, text, n_bytes, n_lines, mem, key, key_len, accept, newlines, ticket, n_records, nullptr);
}
GS_API_CATCH

extern "C" int gs_reads_select_fastq_ml(gs_reads *h, int k, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, const uint8_t *key,
                                        int32_t key_len, uint8_t *accept, uint32_t *newlines, int64_t *n_records, int64_t *consumed_bytes,
                                        int64_t *consumed_lines, int64_t *ticket) try {
    if (!n_records || !consumed_bytes) return fail(GS_E_INVALID, "NULL argument");
    int64_t out[3] = {0, 0, 0};
    const int rc = reads_select(h, k, text, n_bytes, n_lines, mem, key, key_len, accept, newlines, ticket, -1, out);
    return ml_report(rc, out, n_records, consumed_bytes, consumed_lines);
}
GS_API_CATCH

// sizes, offsets, text (gs_launch_rewrite_copy) of the latest chunk's records into slot `slot`, then waits for the totals
static int reads_rewrite(gs_reads *h, GsRewriteParams *R, int slot, size_t bound, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records,
                         int64_t *long_lines) {
    R->out = h->d_out[slot];
    int rc = timer_start(h->timer, h->profile, h->stream);
    if (rc) return rc;
    HIP_TRY(gs_launch_rewrite_copy(R, (int64_t)bound - 64, h->n_cu, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    if ((rc = text_touched(h->text, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(h->h_tot, h->d_tot, sizeof(u64) * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n_bytes = (int64_t)h->h_tot[0];
    if (n_records) *n_records = (int64_t)h->h_tot[1];
    if (long_lines) *long_lines = (int64_t)h->h_tot[2];
    *d_out = *n_bytes > 0 ? h->d_out[slot] : nullptr;
    return GS_OK;
}

// ExtractGoal's readStruct.write on the device: the selected records of the last chunk, four-line FASTQ or FASTA
extern "C" int gs_reads_compact_text(gs_reads *h, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) try {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    TextScan &t = h->text;
    const bool empty = h->last_select && t.last_reads == 0;  // a selected chunk without records: nothing to flag, nothing to write
    if (!empty && (t.tickets == 0 || t.last_four_line)) {
        int rc = timer_start(h->gather_timer, h->profile, h->stream);
        if (rc) return rc;
        if ((rc = text_compact(t, h->stream, 0xff, 1, 0, slot, with_probs, d_out, n_bytes, n_records))) return rc;
        return timer_stop(h->gather_timer, h->profile, h->stream);
    }
    if (!d_out || !n_bytes || !n_records) return fail(GS_E_INVALID, "NULL argument");
    *d_out = nullptr;
    *n_bytes = *n_records = 0;
    if (slot < 0 || slot > 1) return fail(GS_E_INVALID, "slot must be 0 or 1");
    if (h->last_ml) return fail(GS_E_UNSUPPORTED, "records of a general FASTQ chunk are written by the host");
    if (empty) return GS_OK;
    if (!h->d_last_accept) return fail(GS_E_STATE, "the last chunk was submitted without per-read flags");
    if (t.last_reads == 0) return GS_OK;
    const size_t bound = reads_bound(t.last_bytes, t.last_reads);
    int rc = reads_room(h, t.last_reads, slot, bound);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->d_tot, 0, sizeof(u64) * 4, h->stream));
    GsRewriteParams R{};
    reads_params(h, &R);
    R.flags = h->d_last_accept;
    R.flag_mask = 0xff;
    R.flag_want = 1;
    return reads_rewrite(h, &R, slot, bound, d_out, n_bytes, n_records, nullptr);
}
GS_API_CATCH

// the same for the selected records of a FASTA or general FASTQ chunk, the latter with its quality lines where with_probs asks for them
extern "C" int gs_reads_compact_records(gs_reads *h, int with_probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records) try {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return text_records(h->text, h->stream, h->n_cu, 0xff, 1, 1, with_probs, slot, &h->timer, h->profile, d_out, n_bytes, n_records);
}
GS_API_CATCH

extern "C" int gs_reads_fasta2fastq(gs_reads *h, const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem, int slot,
                                    const uint8_t **d_out, int64_t *n_bytes_out, int64_t *long_lines, int64_t *ticket) try {
    if (!h || !d_out || !n_bytes_out) return fail(GS_E_INVALID, "NULL argument");
    *d_out = nullptr;
    *n_bytes_out = 0;
    if (long_lines) *long_lines = 0;
    if (slot < 0 || slot > 1) return fail(GS_E_INVALID, "slot must be 0 or 1");
    if (n_records < 0 || n_bytes < 0 || n_lines < 0 || n_bytes > ((int64_t)1 << 30) || n_records >= ((int64_t)1 << 24))
        return fail(GS_E_INVALID, "bad FASTA chunk (at most 1 GiB and 2^24 - 1 records)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t bound = reads_bound(n_bytes, n_records);
    int rc = reads_room(h, n_records, slot, bound);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->d_tot, 0, sizeof(u64) * 4, h->stream));
    GsRewriteParams R{};
    R.n_lines = n_lines;
    R.n_records = n_records;
    R.goal_mode = 1;
    R.rec_line = h->d_rec_line;
    R.rec_out = (unsigned long long *)h->d_rec_out;
    R.rec_block = (unsigned long long *)h->d_rec_block;
    R.piece_rec = h->d_piece;
    R.totals = (unsigned long long *)h->d_tot;
    h->d_last_accept = nullptr;
    h->last_ml = false;
    h->last_select = false;
    if ((rc = text_submit(h->text, h->stream, text, n_bytes, n_lines, mem, 1, ticket, n_records, nullptr, &R))) return rc;
    return reads_rewrite(h, &R, slot, bound, d_out, n_bytes_out, nullptr, long_lines);
}
GS_API_CATCH

extern "C" int gs_reads_sync(gs_reads *h) {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return GS_OK;
}

// profile != 0: from now on the text kernels of gs_reads_compact_text (FASTA chunks) and gs_reads_fasta2fastq run between events;
// launches / total_ms (either may be NULL): what they add up to so far
extern "C" int gs_reads_kernel_time(gs_reads *h, int profile, int64_t *launches, double *total_ms) {
    int rc = gs_reads_sync(h);
    if (rc) return rc;
    if ((rc = timer_collect(h->timer))) return rc;
    h->profile = profile != 0;
    if (launches) *launches = h->timer.launches;
    if (total_ms) *total_ms = h->timer.total_ms;
    return GS_OK;
}

// what a profiling handle (gs_reads_kernel_time) has measured so far, phase by phase, as time on its stream between events:
// [0] select calls, from the chunk's submission to its flags (the chunk's way in, record search, descriptor compare);
// [1] the four-line gather of gs_reads_compact_text; [2] the FASTA -> FASTQ text kernels (what gs_reads_kernel_time reports)
extern "C" int gs_reads_phase_times(gs_reads *h, int64_t launches[3], double total_ms[3]) {
    if (!launches || !total_ms) return fail(GS_E_INVALID, "NULL argument");
    int rc = gs_reads_sync(h);
    if (rc) return rc;
    KernelTimer *timers[3] = {&h->select_timer, &h->gather_timer, &h->timer};
    for (int i = 0; i < 3; i++) {
        if ((rc = timer_collect(*timers[i]))) return rc;
        launches[i] = timers[i]->launches;
        total_ms[i] = timers[i]->total_ms;
    }
    return GS_OK;
}

extern "C" int gs_reads_get_device(gs_reads *h, int *device) {
    if (!h || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = h->device;
    return GS_OK;
}

extern "C" int gs_reads_text_read_bounds(gs_reads *h, uint64_t *bounds) {
    if (!h || !bounds) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    return text_read_bounds(h->text, h->stream, bounds, "the last chunk was four-line FASTQ: its reads lie in the text (newlines)");
}

extern "C" int gs_reads_text_line_classes(gs_reads *h, uint8_t *classes) {
    if (!h || !classes) return fail(GS_E_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    return text_line_classes(h->text, h->stream, classes);
}

extern "C" int gs_reads_text_wait_copy(gs_reads *h, int64_t ticket) {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return text_wait_copy(h->text, ticket);
}

extern "C" int gs_reads_text_status(gs_reads *h, int64_t *failed_ticket, int64_t *first_bad_record, int64_t totals[3]) {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return text_status(h->text, h->stream, failed_ticket, first_bad_record, totals);
}

extern "C" int gs_reads_text_reset(gs_reads *h, int clear_totals) {
    if (!h) return fail(GS_E_INVALID, "reads is NULL");
    HIP_TRY(hipSetDevice(h->device));
    return text_reset(h->text, clear_totals != 0, h->stream);
}

// ---------------------------------------------------------------------------------------------------
// krakencount: Kraken-style lines counted per tax id (gs_krakencount.hip)
// ---------------------------------------------------------------------------------------------------
#define KC_RING 64  // chunk reports kept
struct gs_krakencount {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t copied = nullptr;
    int64_t max_taxids = 0;
    uint32_t n_slots = 0, slot_bits = 0;
    uint8_t *d_text = nullptr;
    size_t text_cap = 0;
    u64 *d_tile_lt = nullptr, *d_tile_c = nullptr;
    size_t tile_lt_cap = 0, tile_c_cap = 0;
    uint32_t *d_line = nullptr;  // line_end | line_c4 | line_key, line_cap entries each
    size_t line_cap = 0;
    uint32_t *d_keys = nullptr, *d_present = nullptr;
    u64 *d_acc = nullptr, *d_delta = nullptr;
    u64 *d_small = nullptr;  // status, totals, counters, the chunk's report (kc_params)
    u64 *h_res = nullptr;    // KC_RING reports of GS_KC_R_WORDS words, page-locked
    int64_t tickets = 0, absorbed = 0;
    int64_t failed_ticket = -1, failed_line = -1, last_empty = -1;
    int64_t totals[4] = {0, 0, 0, 0};
    bool profile = false;
    KernelTimer timer;
};

enum { KC_S_STATUS = 0, KC_S_CHUNK = 2, KC_S_RUN = 8, KC_S_NKEYS = 12, KC_S_COUNTERS = 13, KC_S_SCAN = 15, KC_S_RESULT = 17, KC_S_WORDS = KC_S_RESULT + GS_KC_R_WORDS };

static void kc_params(gs_krakencount *h, GsKrakenCountParams *P) {
    P->text = h->d_text;
    P->tile_lt = (unsigned long long *)h->d_tile_lt;
    P->tile_c = (unsigned long long *)h->d_tile_c;
    P->scan_tot = (unsigned long long *)h->d_small + KC_S_SCAN;
    P->line_end = h->d_line;
    P->line_c4 = h->d_line + h->line_cap;
    P->line_key = h->d_line + 2 * h->line_cap;
    P->line_cap = (int64_t)h->line_cap;
    P->status = (uint32_t *)(h->d_small + KC_S_STATUS);
    P->chunk_tot = (unsigned long long *)h->d_small + KC_S_CHUNK;
    P->run_tot = (unsigned long long *)h->d_small + KC_S_RUN;
    P->keys = h->d_keys;
    P->present = h->d_present;
    P->acc = (unsigned long long *)h->d_acc;
    P->delta = (unsigned long long *)h->d_delta;
    P->n_slots = h->n_slots;
    P->slot_bits = h->slot_bits;
    P->max_keys = (uint32_t)h->max_taxids;
    P->n_keys = (uint32_t *)(h->d_small + KC_S_NKEYS);
    P->counters = (unsigned long long *)h->d_small + KC_S_COUNTERS;
    P->result = (unsigned long long *)h->d_small + KC_S_RESULT;
}

extern "C" int gs_krakencount_destroy(gs_krakencount *h) {
    if (!h) return GS_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    timer_free(h->timer);
    gs_dev_free(h->d_text);
    gs_dev_free(h->d_tile_lt);
    gs_dev_free(h->d_tile_c);
    gs_dev_free(h->d_line);
    gs_dev_free(h->d_keys);
    gs_dev_free(h->d_present);
    gs_dev_free(h->d_acc);
    gs_dev_free(h->d_delta);
    gs_dev_free(h->d_small);
    if (h->h_res) hipHostFree(h->h_res);
    if (h->copied) hipEventDestroy(h->copied);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
    return GS_OK;
}

static int kc_clear(gs_krakencount *h) {
    GsKrakenCountParams P{};
    kc_params(h, &P);
    HIP_TRY(gs_launch_krakencount_reset(&P, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->absorbed = h->tickets;
    h->failed_ticket = h->failed_line = h->last_empty = -1;
    for (int i = 0; i < 4; i++) h->totals[i] = 0;
    return GS_OK;
}

extern "C" int gs_krakencount_create(gs_krakencount **out, int device, int64_t max_taxids) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (max_taxids < 1 || max_taxids > ((int64_t)1 << 26)) return fail(GS_E_INVALID, "max_taxids must be in [1, 2^26]");
    int rc = use_device(device);
    if (rc) return rc;
    gs_krakencount *h = new gs_krakencount();
    h->device = device;
    h->max_taxids = max_taxids;
    h->slot_bits = 6;  // at most half full
    while (((int64_t)1 << h->slot_bits) < 2 * max_taxids) h->slot_bits++;
    h->n_slots = 1u << h->slot_bits;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->copied, hipEventDisableTiming);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_keys, sizeof(uint32_t) * h->n_slots);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_present, sizeof(uint32_t) * h->n_slots);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_acc, sizeof(u64) * 3 * h->n_slots);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_delta, sizeof(u64) * 3 * h->n_slots);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_small, sizeof(u64) * KC_S_WORDS);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->h_res, sizeof(u64) * KC_RING * GS_KC_R_WORDS);
    if (e != hipSuccess) {
        gs_krakencount_destroy(h);
        return hip_fail(e, "gs_krakencount_create");
    }
    if ((rc = kc_clear(h))) {
        gs_krakencount_destroy(h);
        return rc;
    }
    *out = h;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_krakencount_get_device(gs_krakencount *h, int *device) {
    if (!h || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = h->device;
    return GS_OK;
}

extern "C" int gs_krakencount_geometry(gs_krakencount *h, int64_t geometry[6]) {
    if (!h || !geometry) return fail(GS_E_INVALID, "NULL argument");
    geometry[0] = (int64_t)GS_KC_TILE * GS_KC_GROUP;
    geometry[1] = GS_KC_LDS_SLOTS;
    geometry[2] = h->n_slots;
    geometry[3] = 3;
    geometry[4] = GS_KC_TILE;
    geometry[5] = 1025;  // (gs_launch_scan_blocks: one block of 1024 threads)
    return GS_OK;
}

// the reports the stream has written since the last look (the caller has synchronised it)
static void kc_absorb(gs_krakencount *h) {
    for (; h->absorbed < h->tickets; h->absorbed++) {
        const u64 *R = h->h_res + (size_t)(h->absorbed % KC_RING) * GS_KC_R_WORDS;
        if (R[GS_KC_R_REFUSED] != 0 && h->failed_ticket < 0) {
            h->failed_ticket = h->absorbed;
            h->failed_line = (int64_t)R[GS_KC_R_BAD_LINE];
        }
        h->last_empty = (int64_t)R[GS_KC_R_EMPTY_OFF];
        for (int i = 0; i < 4; i++) h->totals[i] = (int64_t)R[GS_KC_R_RUN + i];
    }
}

static int kc_sync(gs_krakencount *h) {
    if (!h) return fail(GS_E_INVALID, "krakencount is NULL");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    kc_absorb(h);
    return timer_collect(h->timer);
}

extern "C" int gs_krakencount_submit(gs_krakencount *h, const uint8_t *text, int64_t n_bytes, int mem, int64_t *ticket) try {
    if (!h) return fail(GS_E_INVALID, "krakencount is NULL");
    if (n_bytes < 0 || n_bytes > ((int64_t)1 << 30)) return fail(GS_E_INVALID, "a chunk holds at most 1 GiB");
    if (n_bytes > 0 && !text) return fail(GS_E_INVALID, "text is NULL");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (h->tickets - h->absorbed >= KC_RING - 1 && (rc = kc_sync(h))) return rc;
    u64 *res = h->h_res + (size_t)(h->tickets % KC_RING) * GS_KC_R_WORDS;
    if (n_bytes == 0) {  // nothing to count: the report of the chunk in front of it, without its own lines
        if ((rc = kc_sync(h))) return rc;
        const u64 rows = h->tickets ? h->h_res[(size_t)((h->tickets - 1) % KC_RING) * GS_KC_R_WORDS + GS_KC_R_ROWS] : 0;
        for (int i = 0; i < GS_KC_R_WORDS; i++) res[i] = 0;
        res[GS_KC_R_BAD_LINE] = res[GS_KC_R_EMPTY_OFF] = ~0ULL;
        res[GS_KC_R_ROWS] = rows;
        for (int i = 0; i < 4; i++) res[GS_KC_R_RUN + i] = (u64)h->totals[i];
        if (ticket) *ticket = h->tickets;
        h->tickets++;
        return GS_OK;
    }
    const int64_t n_tiles = (n_bytes + GS_KC_TILE - 1) / GS_KC_TILE;
    const size_t padded = (size_t)n_tiles * GS_KC_TILE + 64;
    if ((rc = grow(&h->d_text, &h->text_cap, padded, h->stream))) return rc;
    if ((rc = grow(&h->d_tile_lt, &h->tile_lt_cap, (size_t)n_tiles + 1, h->stream))) return rc;
    if ((rc = grow(&h->d_tile_c, &h->tile_c_cap, (size_t)n_tiles + 1, h->stream))) return rc;
    const size_t lines = (size_t)n_bytes / 7 + 2;  // (a line of the grammar has 7 bytes and more)
    if (h->line_cap < lines) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->line_cap = 0;
        if ((rc = renew(&h->d_line, 3 * (lines + lines / 4)))) return rc;
        h->line_cap = lines + lines / 4;
    }
    HIP_TRY(hipMemcpyAsync(h->d_text, text, (size_t)n_bytes, mem == GS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_text + n_bytes, 0, padded - (size_t)n_bytes, h->stream));
    if (mem == GS_MEM_HOST) {  // the caller's memory is free again on return
        HIP_TRY(hipEventRecord(h->copied, h->stream));
        HIP_TRY(hipEventSynchronize(h->copied));
    }
    GsKrakenCountParams P{};
    kc_params(h, &P);
    P.n_bytes = n_bytes;
    P.n_tiles = n_tiles;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_krakencount(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(res, h->d_small + KC_S_RESULT, sizeof(u64) * GS_KC_R_WORDS, hipMemcpyDeviceToHost, h->stream));
    if (ticket) *ticket = h->tickets;
    h->tickets++;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_krakencount_chunk(gs_krakencount *h, int64_t ticket, int64_t report[8]) {
    if (!h || !report) return fail(GS_E_INVALID, "NULL argument");
    if (ticket < 0 || ticket >= h->tickets || ticket < h->tickets - (KC_RING - 1)) return fail(GS_E_INVALID, "no report is kept for this ticket");
    int rc = kc_sync(h);
    if (rc) return rc;
    const u64 *R = h->h_res + (size_t)(ticket % KC_RING) * GS_KC_R_WORDS;
    for (int i = 0; i < 8; i++) report[i] = (int64_t)R[i];
    return GS_OK;
}

extern "C" int gs_krakencount_status(gs_krakencount *h, int64_t *failed_ticket, int64_t *first_bad_line, int64_t *first_empty_offset, int64_t totals[4]) {
    int rc = kc_sync(h);
    if (rc) return rc;
    if (failed_ticket) *failed_ticket = h->failed_ticket;
    if (first_bad_line) *first_bad_line = h->failed_line;
    if (first_empty_offset) *first_empty_offset = h->last_empty;
    if (totals)
        for (int i = 0; i < 4; i++) totals[i] = h->totals[i];
    return GS_OK;
}

extern "C" int gs_krakencount_reset(gs_krakencount *h) {
    int rc = kc_sync(h);
    if (rc) return rc;
    return kc_clear(h);
}

extern "C" int gs_krakencount_fetch(gs_krakencount *h, int32_t *taxids, int64_t *counts, int64_t cap, int64_t *n_rows) try {
    if (!n_rows) return fail(GS_E_INVALID, "n_rows is NULL");
    int rc = kc_sync(h);
    if (rc) return rc;
    std::vector<uint32_t> keys(h->n_slots), present(h->n_slots);
    std::vector<u64> acc((size_t)h->n_slots * 3);
    HIP_TRY(hipMemcpy(keys.data(), h->d_keys, sizeof(uint32_t) * h->n_slots, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(present.data(), h->d_present, sizeof(uint32_t) * h->n_slots, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(acc.data(), h->d_acc, sizeof(u64) * 3 * h->n_slots, hipMemcpyDeviceToHost));
    std::vector<std::pair<std::string, uint32_t>> rows;  // (decimal string, slot): DigitTrie.collect visits a prefix before its extensions
    for (uint32_t s = 0; s < h->n_slots; s++)
        if (keys[s] != GS_KC_EMPTY && present[s]) rows.push_back({std::to_string(keys[s]), s});
    std::sort(rows.begin(), rows.end());
    *n_rows = (int64_t)rows.size();
    if (cap < *n_rows) return GS_OK;
    if (!rows.empty() && (!taxids || !counts)) return fail(GS_E_INVALID, "NULL argument");
    for (size_t i = 0; i < rows.size(); i++) {
        taxids[i] = (int32_t)keys[rows[i].second];
        for (int j = 0; j < 3; j++) counts[3 * i + j] = (int64_t)acc[(size_t)rows[i].second * 3 + j];
    }
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_krakencount_counters(gs_krakencount *h, int64_t counters[2]) {
    if (!counters) return fail(GS_E_INVALID, "NULL argument");
    int rc = kc_sync(h);
    if (rc) return rc;
    u64 c[2];
    HIP_TRY(hipMemcpy(c, h->d_small + KC_S_COUNTERS, sizeof(c), hipMemcpyDeviceToHost));
    counters[0] = (int64_t)c[0];
    counters[1] = (int64_t)c[1];
    return GS_OK;
}

extern "C" int gs_krakencount_kernel_time(gs_krakencount *h, int profile, int64_t *launches, double *total_ms) {
    int rc = kc_sync(h);
    if (rc) return rc;
    h->profile = profile != 0;
    if (launches) *launches = h->timer.launches;
    if (total_ms) *total_ms = h->timer.total_ms;
    return GS_OK;
}

// ---------------------------------------------------------------------------------------------------
// chunks of whole lines: what the accmap, asmsum and taxtree handles share
// ---------------------------------------------------------------------------------------------------
// What the handles that take chunks of whole lines share (gs_accmap, gs_asmsum, gs_taxtree): the stream, the padded text of the chunk
// under way, the scan words of its tiles, the small words -- the first of them the status: bad line | longest line << 32 -- and the
// kernel timer.  Each handle is one of these in front of its own members.
struct LineStage {
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t *d_text = nullptr;
    size_t text_cap = 0;
    u64 *d_tile = nullptr;  // tile_cap entries per scan word
    uint32_t *d_tail = nullptr;
    size_t tile_cap = 0;
    u64 *d_small = nullptr;
    bool profile = false;
    KernelTimer timer;
};
enum { LINES_SMALL_MAX = 16 };  // the small words a chunk resets are fewer

static void lines_free(LineStage &s) {
    timer_free(s.timer);
    for (void *p : {(void *)s.d_text, (void *)s.d_tile, (void *)s.d_tail, (void *)s.d_small}) gs_dev_free(p);
    if (s.stream) hipStreamDestroy(s.stream);
}

// the argument checks in front of a chunk; the handle's own checks (its state, host only) follow them in its entry point
static int lines_args(const void *h, const uint8_t *text, int64_t n_bytes, int mem, const int64_t *report) {
    if (!h || !report) return fail(GS_E_INVALID, "NULL argument");
    if (n_bytes < 0 || n_bytes > ((int64_t)1 << 30)) return fail(GS_E_INVALID, "a chunk holds at most 1 GiB");
    if (n_bytes > 0 && !text) return fail(GS_E_INVALID, "text is NULL");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    return GS_OK;
}

// The opening of a chunk: the report of an empty chunk; then, unless the chunk is empty, room for its text in tiles of `tile` bytes and
// for `words` scan words per tile, the text behind zero padding, and the first n_small small words reset with `none` as the bad line.
static int lines_open(LineStage &s, const uint8_t *text, int64_t n_bytes, int mem, int64_t report[8], int tile, int words, uint32_t none, int n_small,
                      int64_t *tiles) {
    for (int i = 0; i < 8; i++) report[i] = 0;
    report[4] = -1;
    if (n_bytes == 0) return GS_OK;
    HIP_TRY(hipSetDevice(s.device));
    const int64_t n_tiles = *tiles = (n_bytes + tile - 1) / tile;
    const size_t padded = (size_t)n_tiles * (size_t)tile + 64;
    int rc;
    if ((rc = grow(&s.d_text, &s.text_cap, padded, s.stream))) return rc;
    if (s.tile_cap < (size_t)n_tiles + 1) {
        const size_t cap = (size_t)n_tiles + 1 + (size_t)n_tiles / 4;
        HIP_TRY(hipStreamSynchronize(s.stream));
        s.tile_cap = 0;
        if ((rc = renew(&s.d_tile, (size_t)words * cap))) return rc;
        if ((rc = renew(&s.d_tail, cap))) return rc;
        s.tile_cap = cap;
    }
    HIP_TRY(hipMemcpyAsync(s.d_text, text, (size_t)n_bytes, mem == GS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s.stream));
    HIP_TRY(hipMemsetAsync(s.d_text + n_bytes, 0, padded - (size_t)n_bytes, s.stream));
    u64 small[LINES_SMALL_MAX] = {};
    small[0] = (u64)none;  // bad line: none; longest line: 0
    HIP_TRY(hipMemcpy(s.d_small, small, (size_t)n_small * sizeof(u64), hipMemcpyHostToDevice));  // (the stream is idle between calls)
    return GS_OK;
}

// the verdict of a chunk out of its status word: report[5] its longest line, and of a refused chunk report[3] and the bad line in
// report[4].  true: refused
static bool lines_refused(u64 status, uint32_t none, int64_t report[8]) {
    const uint32_t bad = (uint32_t)status;
    report[5] = (int64_t)(status >> 32);
    if (bad == none) return false;
    report[3] = 1;
    report[4] = (int64_t)bad;
    return true;
}

// the kernel time so far, and whether the launches from here on are timed
static int lines_kernel_time(LineStage &s, bool host_only, int profile, int64_t *launches, double *total_ms) {
    if (host_only) {
        if (launches) *launches = 0;
        if (total_ms) *total_ms = 0;
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(s.device));
    HIP_TRY(hipStreamSynchronize(s.stream));
    int rc = timer_collect(s.timer);
    if (rc) return rc;
    s.profile = profile != 0;
    if (launches) *launches = s.timer.launches;
    if (total_ms) *total_ms = s.timer.total_ms;
    return GS_OK;
}

static int lines_get_device(const LineStage *s, int *device) {
    if (!s || !device) return fail(GS_E_INVALID, "NULL argument");
    *device = s->device;
    return GS_OK;
}

// Room for `need` elements in all in every array of a set that shares one capacity, by doubling; the first `used` elements of each
// stay.  All or nothing: no array of the set has moved when this fails.  `what` names the arrays in the failure's message.
struct KeptArray {
    void **p;
    size_t elem;  // bytes per element
};
static int grow_keep(std::initializer_list<KeptArray> arrays, size_t *cap, size_t used, size_t need, hipStream_t stream, const char *what) {
    if (need <= *cap) return GS_OK;
    const size_t n = std::max(need, 2 * *cap);
    std::vector<void *> fresh(arrays.size(), nullptr);
    hipError_t e = hipSuccess;
    size_t i = 0;
    for (const KeptArray &a : arrays) {
        if (e == hipSuccess) e = gs_dev_alloc(&fresh[i], n * a.elem);
        if (e == hipSuccess && used) e = hipMemcpyAsync(fresh[i], *a.p, used * a.elem, hipMemcpyDeviceToDevice, stream);
        i++;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        for (void *p : fresh) gs_dev_free(p);
        return hip_fail(e, what);
    }
    i = 0;
    for (const KeptArray &a : arrays) {
        gs_dev_free(*a.p);
        *a.p = fresh[i++];
    }
    *cap = n;
    return GS_OK;
}
template <typename T>
static int grow_keep(T **p, size_t *cap, size_t used, size_t need, hipStream_t stream, const char *what) {
    return grow_keep({{(void **)p, sizeof(T)}}, cap, used, need, stream, what);
}

// ---------------------------------------------------------------------------------------------------
// accmap: RefSeq catalog lines to the accession map (gs_accmap.hip)
// ---------------------------------------------------------------------------------------------------
struct gs_accmap : LineStage {
    bool finished = false;
    int32_t dna = 0, rna = 0, mrna = 0, n_cat = 0, n_stat = 0, n_nodes = 0;
    GsAccmapPatterns *d_pat = nullptr;
    int32_t *d_known = nullptr, *d_regions = nullptr;  // (d_tile: tile_lt | tile_put)
    uint8_t *d_keys = nullptr;  // entry_cap slots of 32 bytes; sorted once finished
    int32_t *d_nodes = nullptr;
    size_t entry_cap = 0;
    int64_t n_entries = 0, n_passing = 0;
    std::vector<int32_t> host_regions;  // the entries that came in through gs_accmap_append, per node
    bool host_only = false;             // device == -1: no device is touched; the entries live in h_keys / h_nodes, sorted once finished
    std::vector<uint8_t> h_keys;
    std::vector<int32_t> h_nodes;
};
// d_small: status, chunk counters, scan sums, finish counts, flag
enum { AM_S_STATUS = 0, AM_S_CHUNK = 1, AM_S_SCAN = AM_S_CHUNK + GS_AM_C_WORDS, AM_S_COUNTS = AM_S_SCAN + 2, AM_S_FLAG = AM_S_COUNTS + 2, AM_S_WORDS };
static_assert(GS_AM_WORDS == 2 && AM_S_STATUS == 0 && AM_S_SCAN <= LINES_SMALL_MAX, "the status words fill the first 64-bit word of d_small");

extern "C" int gs_accmap_destroy(gs_accmap *h) try {
    if (!h) return GS_OK;
    if (h->host_only) {
        delete h;
        return GS_OK;
    }
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void *p : {(void *)h->d_pat, (void *)h->d_known, (void *)h->d_regions, (void *)h->d_keys, (void *)h->d_nodes}) gs_dev_free(p);
    lines_free(*h);
    delete h;
    return GS_OK;
}
GS_API_CATCH

// room for `need` entries in all; what is there stays
static int am_entry_room(gs_accmap *h, size_t need) {
    if (need > h->entry_cap && need > ((size_t)1 << 31)) return fail(GS_E_UNSUPPORTED, "an accession map holds at most 2^31 entries");
    return grow_keep({{(void **)&h->d_keys, 32}, {(void **)&h->d_nodes, sizeof(int32_t)}}, &h->entry_cap, (size_t)h->n_entries, need, h->stream,
                     "gs_accmap: growing the entry arrays");
}

extern "C" int gs_accmap_create(gs_accmap **out, int device, const gs_accmap_cfg *cfg) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(GS_E_INVALID, "cfg is NULL");
    if (cfg->n_categories < 1 || cfg->n_categories > GS_AM_MAX_PATTERNS || cfg->n_statuses < 1 || cfg->n_statuses > GS_AM_MAX_PATTERNS)
        return fail(GS_E_INVALID, "1 to 16 category strings and 1 to 16 status strings");
    if (!cfg->categories || !cfg->statuses) return fail(GS_E_INVALID, "categories or statuses is NULL");
    if (cfg->n_nodes < 0 || (cfg->n_nodes > 0 && !cfg->known_taxids)) return fail(GS_E_INVALID, "known_taxids is NULL or n_nodes < 0");
    if (cfg->reserve_entries < 0 || cfg->reserve_entries > ((int64_t)1 << 31)) return fail(GS_E_INVALID, "reserve_entries must be in [0, 2^31]");
    for (int32_t i = 0; i < cfg->n_nodes; i++)
        if (cfg->known_taxids[i] <= 0 || (i && cfg->known_taxids[i] <= cfg->known_taxids[i - 1]))
            return fail(GS_E_INVALID, "known_taxids must be positive, ascending and distinct");
    GsAccmapPatterns pat{};
    for (int kind = 0; kind < 2; kind++) {
        const int n = kind ? cfg->n_statuses : cfg->n_categories;
        for (int i = 0; i < n; i++) {
            const char *s = (kind ? cfg->statuses : cfg->categories)[i];
            const size_t len = s ? strnlen(s, GS_AM_MAX_PATTERN + 1) : 0;
            if (len < 1 || len > GS_AM_MAX_PATTERN) return fail(GS_E_INVALID, "a category or status string has 1 to 32 bytes");
            pat.len[kind * GS_AM_MAX_PATTERNS + i] = (uint8_t)len;
            memcpy(pat.text[kind * GS_AM_MAX_PATTERNS + i], s, len);
        }
    }
    int rc = device == -1 ? (int)GS_OK : use_device(device);
    if (rc) return rc;
    gs_accmap *h = new gs_accmap();
    h->device = device;
    h->host_only = device == -1;
    h->dna = cfg->dna != 0;
    h->rna = cfg->rna != 0;
    h->mrna = cfg->mrna != 0;
    h->n_cat = cfg->n_categories;
    h->n_stat = cfg->n_statuses;
    h->n_nodes = cfg->n_nodes;
    h->host_regions.assign((size_t)cfg->n_nodes, 0);
    if (h->host_only) {
        *out = h;
        return GS_OK;
    }
    const size_t nodes = (size_t)std::max(cfg->n_nodes, 1);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_pat, sizeof(GsAccmapPatterns));
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_known, sizeof(int32_t) * nodes);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_regions, sizeof(int32_t) * nodes);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_small, sizeof(u64) * AM_S_WORDS);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_pat, &pat, sizeof(pat), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && cfg->n_nodes) e = hipMemcpyAsync(h->d_known, cfg->known_taxids, sizeof(int32_t) * nodes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_regions, 0, sizeof(int32_t) * nodes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (pat is a local)
    if (e != hipSuccess) {
        gs_accmap_destroy(h);
        return hip_fail(e, "gs_accmap_create");
    }
    if ((rc = am_entry_room(h, (size_t)std::max<int64_t>(cfg->reserve_entries, 1)))) {
        gs_accmap_destroy(h);
        return rc;
    }
    *out = h;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_accmap_get_device(gs_accmap *h, int *device) try {
    return lines_get_device(h, device);
}
GS_API_CATCH

extern "C" int gs_accmap_get_n_nodes(gs_accmap *h, int32_t *n_nodes) try {
    if (!h || !n_nodes) return fail(GS_E_INVALID, "NULL argument");
    *n_nodes = h->n_nodes;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_accmap_submit(gs_accmap *h, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]) try {
    int rc = lines_args(h, text, n_bytes, mem, report);
    if (rc) return rc;
    if (h->finished) return fail(GS_E_STATE, "gs_accmap_submit comes in front of gs_accmap_finish");
    if (h->host_only) return fail(GS_E_UNSUPPORTED, "a host-only accession map (device -1) takes entries through gs_accmap_append alone");
    int64_t n_tiles = 0;
    u64 small[AM_S_SCAN];
    rc = lines_open(*h, text, n_bytes, mem, report, GS_AM_TILE, 2, GS_AM_NONE, AM_S_SCAN, &n_tiles);  // (tile_lt | tile_put)
    if (rc || n_bytes == 0) return rc;
    GsAccmapParams P{};
    P.text = h->d_text;
    P.n_bytes = n_bytes;
    P.n_tiles = n_tiles;
    P.last = last != 0;
    P.dna = h->dna;
    P.rna = h->rna;
    P.mrna = h->mrna;
    P.n_cat = h->n_cat;
    P.n_stat = h->n_stat;
    P.pat = h->d_pat;
    P.known = h->d_known;
    P.n_nodes = h->n_nodes;
    P.tile_lt = (unsigned long long *)h->d_tile;
    P.tile_put = (unsigned long long *)h->d_tile + h->tile_cap;
    P.tile_tail = h->d_tail;
    P.scan_tot = (unsigned long long *)h->d_small + AM_S_SCAN;
    P.status = (uint32_t *)(h->d_small + AM_S_STATUS);
    P.chunk = (unsigned long long *)h->d_small + AM_S_CHUNK;
    P.regions = h->d_regions;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_accmap_count(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(small, h->d_small, sizeof(small), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the one wait of a chunk: its verdict and its counts, between the passes
    report[0] = (int64_t)small[AM_S_CHUNK + GS_AM_C_LINES];
    if (lines_refused(small[AM_S_STATUS], GS_AM_NONE, report)) return timer_collect(h->timer);
    const int64_t n_put = (int64_t)small[AM_S_CHUNK + GS_AM_C_PUT];
    report[1] = (int64_t)small[AM_S_CHUNK + GS_AM_C_PASSING];
    report[2] = n_put;
    if (n_put > 0) {
        if ((rc = am_entry_room(h, (size_t)(h->n_entries + n_put)))) return rc;
        P.keys = h->d_keys;
        P.nodes = h->d_nodes;
        P.first_entry = h->n_entries;
        P.entry_cap = (int64_t)h->entry_cap;
        if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
        HIP_TRY(gs_launch_accmap_write(&P, h->stream));
        if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->n_entries += n_put;
    h->n_passing += report[1];
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_accmap_append(gs_accmap *h, const uint8_t *keys32, const int32_t *nodes, int64_t n, int64_t n_passing) try {
    if (!h) return fail(GS_E_INVALID, "accmap is NULL");
    if (n < 0 || n_passing < n) return fail(GS_E_INVALID, "n < 0 or n_passing < n");
    if (n > 0 && (!keys32 || !nodes)) return fail(GS_E_INVALID, "NULL argument");
    if (h->finished) return fail(GS_E_STATE, "gs_accmap_append comes in front of gs_accmap_finish");
    for (int64_t i = 0; i < n; i++) {
        if (nodes[i] < 0 || nodes[i] >= h->n_nodes) return fail(GS_E_INVALID, "a node is no index into known_taxids");
        const uint8_t *k = keys32 + 32 * i;
        bool ok = k[0] <= GS_AM_MAX_KEY;
        for (int j = 1; j < 32 && ok; j++) ok = j <= k[0] ? k[j] < 0x80 : k[j] == 0;
        if (!ok) return fail(GS_E_INVALID, "a slot is a length of 0..31, that many bytes below 0x80, and zeros");
    }
    if (n > 0 && h->host_only) {
        h->h_keys.insert(h->h_keys.end(), keys32, keys32 + 32 * n);
        h->h_nodes.insert(h->h_nodes.end(), nodes, nodes + n);
        for (int64_t i = 0; i < n; i++) h->host_regions[(size_t)nodes[i]]++;
        h->n_entries += n;
    } else if (n > 0) {
        HIP_TRY(hipSetDevice(h->device));
        int rc = am_entry_room(h, (size_t)(h->n_entries + n));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(h->d_keys + (size_t)h->n_entries * 32, keys32, (size_t)n * 32, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->d_nodes + h->n_entries, nodes, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int64_t i = 0; i < n; i++) h->host_regions[(size_t)nodes[i]]++;
        h->n_entries += n;
    }
    h->n_passing += n_passing;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_accmap_finish(gs_accmap *h, int64_t info[4]) try {
    if (!h || !info) return fail(GS_E_INVALID, "NULL argument");
    if (h->finished) return fail(GS_E_STATE, "gs_accmap_finish was called before");
    if (h->host_only) {  // the same order: bytes below 0x80, so the slots compare as their big-endian words do
        const int64_t n = h->n_entries;
        std::vector<uint32_t> seq((size_t)n);
        for (int64_t i = 0; i < n; i++) seq[(size_t)i] = (uint32_t)i;
        const uint8_t *k = h->h_keys.data();
        std::stable_sort(seq.begin(), seq.end(), [k](uint32_t a, uint32_t b) { return memcmp(k + 32 * (size_t)a, k + 32 * (size_t)b, 32) < 0; });
        std::vector<uint8_t> keys((size_t)n * 32);
        std::vector<int32_t> nodes((size_t)n);
        info[2] = info[3] = 0;
        for (int64_t i = 0; i < n; i++) {
            memcpy(keys.data() + 32 * (size_t)i, k + 32 * (size_t)seq[(size_t)i], 32);
            nodes[(size_t)i] = h->h_nodes[seq[(size_t)i]];
            if (i && memcmp(keys.data() + 32 * (size_t)i, keys.data() + 32 * (size_t)(i - 1), 32) == 0) {
                info[2]++;
                info[3] += nodes[(size_t)i] != nodes[(size_t)i - 1];
            }
        }
        h->h_keys.swap(keys);
        h->h_nodes.swap(nodes);
        h->finished = true;
        info[0] = n;
        info[1] = h->n_passing;
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    const int64_t n = h->n_entries;
    const size_t room = (size_t)std::max<int64_t>(n, 1);
    size_t tmp_bytes = 0;
    HIP_TRY(gs_accmap_sort_bytes(n, &tmp_bytes));
    u64 *word = nullptr;      // word | word_alt
    uint32_t *seq = nullptr;  // seq | seq_alt
    void *tmp = nullptr;
    uint8_t *keys = nullptr;
    int32_t *nodes = nullptr;
    hipError_t e = gs_dev_alloc(&word, 2 * room * sizeof(u64));
    if (e == hipSuccess) e = gs_dev_alloc(&seq, 2 * room * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1));
    if (e == hipSuccess) e = gs_dev_alloc(&keys, room * 32);
    if (e == hipSuccess) e = gs_dev_alloc(&nodes, room * sizeof(int32_t));
    int rc = e == hipSuccess ? timer_start(h->timer, h->profile, h->stream) : hip_fail(e, "gs_accmap_finish");
    uint32_t *seq_sorted = nullptr;
    u64 counts[2] = {0, 0};
    if (!rc) {
        e = gs_accmap_sort_entries(h->d_keys, h->d_nodes, n, word, word + room, seq, seq + room, tmp, tmp_bytes, (uint32_t *)(h->d_small + AM_S_FLAG), keys, nodes,
                             &seq_sorted, (unsigned long long *)h->d_small + AM_S_COUNTS, h->stream);
        if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(counts, h->d_small + AM_S_COUNTS, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = hip_fail(e, "gs_accmap_finish");
    }
    gs_dev_free(word);
    gs_dev_free(seq);
    gs_dev_free(tmp);
    if (rc) {
        gs_dev_free(keys);
        gs_dev_free(nodes);
        return rc;
    }
    gs_dev_free(h->d_keys);
    gs_dev_free(h->d_nodes);
    h->d_keys = keys;
    h->d_nodes = nodes;
    h->entry_cap = room;
    h->finished = true;
    info[0] = n;
    info[1] = h->n_passing;
    info[2] = (int64_t)counts[0];
    info[3] = (int64_t)counts[1];
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_accmap_fetch(gs_accmap *h, uint8_t *keys32, int32_t *nodes, int32_t *regions) try {
    if (!h) return fail(GS_E_INVALID, "accmap is NULL");
    if (!h->finished) return fail(GS_E_STATE, "gs_accmap_fetch comes behind gs_accmap_finish");
    if (h->host_only) {
        if (keys32 && h->n_entries) memcpy(keys32, h->h_keys.data(), h->h_keys.size());
        if (nodes && h->n_entries) memcpy(nodes, h->h_nodes.data(), h->h_nodes.size() * sizeof(int32_t));
        if (regions && h->n_nodes) memcpy(regions, h->host_regions.data(), h->host_regions.size() * sizeof(int32_t));
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (keys32 && h->n_entries) HIP_TRY(hipMemcpy(keys32, h->d_keys, (size_t)h->n_entries * 32, hipMemcpyDeviceToHost));
    if (nodes && h->n_entries) HIP_TRY(hipMemcpy(nodes, h->d_nodes, (size_t)h->n_entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (regions && h->n_nodes) {
        HIP_TRY(hipMemcpy(regions, h->d_regions, (size_t)h->n_nodes * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t i = 0; i < h->n_nodes; i++) regions[i] += h->host_regions[(size_t)i];
    }
    return GS_OK;
}
GS_API_CATCH

// node_out[n] (device) for the n header lines at d_headers / d_off (device)
static int am_lookup_device(gs_accmap *h, const uint8_t *d_headers, const u64 *d_off, int64_t n, int complete_only, int32_t *d_out, hipStream_t stream) {
    int rc = timer_start(h->timer, h->profile, stream);
    if (rc) return rc;
    HIP_TRY(gs_launch_accmap_lookup(d_headers, d_off, n, complete_only != 0, h->d_keys, h->d_nodes, h->n_entries, d_out, stream));
    return timer_stop(h->timer, h->profile, stream);
}

extern "C" int gs_accmap_lookup(gs_accmap *h, const uint8_t *headers, const uint64_t *header_off, int64_t n, int mem, int complete_only,
                                int32_t *node_out) try {
    if (!h) return fail(GS_E_INVALID, "accmap is NULL");
    if (n < 0) return fail(GS_E_INVALID, "n < 0");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (!header_off || (n > 0 && (!headers || !node_out))) return fail(GS_E_INVALID, "NULL argument");
    if (!h->finished) return fail(GS_E_STATE, "gs_accmap_lookup comes behind gs_accmap_finish");
    if (n == 0) return GS_OK;
    if (h->host_only) {  // gs_am_lookup_kernel, line by line
        if (mem != GS_MEM_HOST) return fail(GS_E_UNSUPPORTED, "a host-only accession map looks up host memory alone");
        for (int64_t i = 0; i < n; i++) {
            const uint8_t *line = headers + header_off[i];
            const size_t size = (size_t)(header_off[i + 1] - header_off[i]);
            const uint8_t *blank = size ? (const uint8_t *)memchr(line, ' ', size) : nullptr;
            node_out[i] = -1;
            const int64_t len = blank ? blank - line - 1 : -1;
            if (len < 0 || len > GS_AM_MAX_KEY) continue;
            if (complete_only) {
                bool ok = false;
                for (const char *pre : {"AC_", "NC_", "NZ_", "NM_", "XM_", "NR_", "XR_"}) ok = ok || (len >= 3 && memcmp(line + 1, pre, 3) == 0);
                if (!ok) continue;
            }
            uint8_t probe[32] = {(uint8_t)len};
            memcpy(probe + 1, line + 1, (size_t)len);
            int64_t lo = 0, hi = h->n_entries;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (memcmp(h->h_keys.data() + 32 * (size_t)mid, probe, 32) < 0)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < h->n_entries && memcmp(h->h_keys.data() + 32 * (size_t)lo, probe, 32) == 0) node_out[i] = h->h_nodes[(size_t)lo];
        }
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (mem == GS_MEM_DEVICE) {
        if ((rc = am_lookup_device(h, headers, (const u64 *)header_off, n, complete_only, node_out, h->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        return timer_collect(h->timer);
    }
    for (int64_t i = 0; i < n; i++)
        if (header_off[i + 1] < header_off[i]) return fail(GS_E_INVALID, "header_off must ascend");
    const size_t n_bytes = (size_t)(header_off[n] - header_off[0]);
    uint8_t *d_headers = nullptr;
    u64 *d_off = nullptr;
    int32_t *d_out = nullptr;
    hipError_t e = gs_dev_alloc(&d_headers, std::max<size_t>(n_bytes, 1));
    if (e == hipSuccess) e = gs_dev_alloc(&d_off, ((size_t)n + 1) * sizeof(u64));
    if (e == hipSuccess) e = gs_dev_alloc(&d_out, (size_t)n * sizeof(int32_t));
    std::vector<u64> off0((size_t)n + 1);  // the offsets from 0: the copy holds the header bytes alone
    for (int64_t i = 0; i <= n; i++) off0[(size_t)i] = header_off[i] - header_off[0];
    if (e == hipSuccess && n_bytes) e = hipMemcpyAsync(d_headers, headers + header_off[0], n_bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off0.data(), ((size_t)n + 1) * sizeof(u64), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (off0 is a local)
    rc = e == hipSuccess ? am_lookup_device(h, d_headers, d_off, n, complete_only, d_out, h->stream) : hip_fail(e, "gs_accmap_lookup");
    if (!rc) {
        e = hipMemcpyAsync(node_out, d_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = hip_fail(e, "gs_accmap_lookup");
    } else {
        hipStreamSynchronize(h->stream);
    }
    gs_dev_free(d_headers);
    gs_dev_free(d_off);
    gs_dev_free(d_out);
    return rc ? rc : timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_accmap_lookup_genomes(gs_accmap *h, gs_genomes *g, int complete_only, int32_t *node_out) try {
    if (!h || !g) return fail(GS_E_INVALID, "NULL argument");
    if (!h->finished) return fail(GS_E_STATE, "gs_accmap_lookup_genomes comes behind gs_accmap_finish");
    if (h->host_only) return fail(GS_E_UNSUPPORTED, "a host-only accession map looks up host memory alone");
    if (g->state < 1) return fail(GS_E_STATE, "gs_accmap_lookup_genomes comes behind a gs_genomes_scan that took its chunk");
    if (g->device != h->device) return fail(GS_E_INVALID, "the genomes handle lives on another device");
    if (g->n_records == 0) return GS_OK;
    if (!node_out) return fail(GS_E_INVALID, "node_out is NULL");
    GsGenomesParams P{};
    int rc = gn_device_headers(g, &P);
    if (rc) return rc;
    int32_t *d_out = nullptr;
    HIP_TRY(gs_dev_alloc(&d_out, (size_t)g->n_records * sizeof(int32_t)));
    // (on the genomes handle's stream, behind its header kernel; the map is at rest once finished)
    rc = am_lookup_device(h, g->d_hdr, (const u64 *)P.hdr_off, g->n_records, complete_only, d_out, g->stream);
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(node_out, d_out, (size_t)g->n_records * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    gs_dev_free(d_out);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "gs_accmap_lookup_genomes");
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_accmap_kernel_time(gs_accmap *h, int profile, int64_t *launches, double *total_ms) try {
    if (!h) return fail(GS_E_INVALID, "accmap is NULL");
    return lines_kernel_time(*h, h->host_only, profile, launches, total_ms);
}
GS_API_CATCH

// ---------------------------------------------------------------------------------------------------
// asmsum: Genbank assembly summary lines to the picks per tree node (gs_asmsum.hip, gs_asmsumparse.h)
// ---------------------------------------------------------------------------------------------------
struct gs_asmsum : LineStage {
    bool finished = false;
    bool host_only = false;  // device == -1: no device is touched; the entries live in `store`
    int32_t n_nodes = 0, quality_mask = -1, reference_only = 0, key_field = 5;
    int32_t *d_known = nullptr;
    uint8_t *d_filter = nullptr;  // nullptr: every node
    uint16_t *d_slots = nullptr;  // per line of a chunk: its slot, its high-byte mark, its verdict
    uint8_t *d_high = nullptr;
    u64 *d_verdict = nullptr;
    size_t line_cap = 0;
    u64 *d_line_blk = nullptr;
    size_t blk_cap = 0;
    uint32_t *d_put_line = nullptr;
    size_t put_cap = 0;
    GsAsmEntry *d_entries = nullptr;  // kept entries in input order; their strings in d_pool
    size_t entry_cap = 0;
    uint8_t *d_pool = nullptr;
    size_t pool_cap = 0;
    int64_t n_entries = 0, pool_used = 0, n_counted = 0, n_lines = 0;
    // finished: the picked entries, nodes ascending
    int64_t n_picked = 0, nodes_with_entries = 0, out_pool_bytes = 0;
    GsAsmEntry *d_out = nullptr;
    u64 *d_str_off = nullptr;
    uint8_t *d_out_pool = nullptr;
    gs_host::AsmsumStore store;
};
// d_small: status, chunk counters, scan sums, finish counts
enum { AS_S_STATUS = 0, AS_S_CHUNK = 1, AS_S_SCAN = AS_S_CHUNK + GS_AS_C_WORDS, AS_S_COUNTS = AS_S_SCAN + 2, AS_S_WORDS = AS_S_COUNTS + 2 };
static_assert(GS_AS_WORDS == 2 && AS_S_STATUS == 0 && AS_S_COUNTS <= LINES_SMALL_MAX, "the status words fill the first 64-bit word of d_small");

extern "C" int gs_asmsum_destroy(gs_asmsum *h) try {
    if (!h) return GS_OK;
    if (h->host_only) {
        delete h;
        return GS_OK;
    }
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void *p : {(void *)h->d_known, (void *)h->d_filter, (void *)h->d_slots, (void *)h->d_high, (void *)h->d_verdict, (void *)h->d_line_blk,
                    (void *)h->d_put_line, (void *)h->d_entries, (void *)h->d_pool, (void *)h->d_out, (void *)h->d_str_off, (void *)h->d_out_pool})
        gs_dev_free(p);
    lines_free(*h);
    delete h;
    return GS_OK;
}
GS_API_CATCH

static int as_entry_room(gs_asmsum *h, int64_t more_entries, int64_t more_bytes) {
    if (h->n_entries + more_entries > ((int64_t)1 << 31)) return fail(GS_E_UNSUPPORTED, "an assembly summary handle holds at most 2^31 entries");
    const char *what = "gs_asmsum: growing the entry arrays";
    int rc = grow_keep(&h->d_entries, &h->entry_cap, (size_t)h->n_entries, (size_t)(h->n_entries + more_entries), h->stream, what);
    if (!rc) rc = grow_keep(&h->d_pool, &h->pool_cap, (size_t)h->pool_used, (size_t)(h->pool_used + more_bytes), h->stream, what);
    return rc;
}

extern "C" int gs_asmsum_create(gs_asmsum **out, int device, const gs_asmsum_cfg *cfg) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(GS_E_INVALID, "cfg is NULL");
    if (cfg->n_nodes < 0 || (cfg->n_nodes > 0 && !cfg->known_taxids)) return fail(GS_E_INVALID, "known_taxids is NULL or n_nodes < 0");
    if (cfg->reserve_entries < 0 || cfg->reserve_entries > ((int64_t)1 << 31)) return fail(GS_E_INVALID, "reserve_entries must be in [0, 2^31]");
    if (cfg->quality_mask != -1 && (cfg->quality_mask & ~0x7ff)) return fail(GS_E_INVALID, "quality_mask is -1 or has bits 0..10 alone");
    for (int32_t i = 0; i < cfg->n_nodes; i++)
        if (cfg->known_taxids[i] <= 0 || cfg->known_taxids[i] > 999999999 || (i && cfg->known_taxids[i] <= cfg->known_taxids[i - 1]))
            return fail(GS_E_INVALID, "known_taxids must be positive, ascending, distinct and of at most 9 digits");
    int rc = device == -1 ? (int)GS_OK : use_device(device);
    if (rc) return rc;
    gs_asmsum *h = new gs_asmsum();
    h->device = device;
    h->host_only = device == -1;
    h->n_nodes = cfg->n_nodes;
    h->quality_mask = cfg->quality_mask;
    h->reference_only = cfg->reference_only != 0;
    h->key_field = cfg->use_species_taxid ? 6 : 5;
    if (h->host_only) {
        *out = h;
        return GS_OK;
    }
    const size_t nodes = (size_t)std::max(cfg->n_nodes, 1);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_known, sizeof(int32_t) * nodes);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_small, sizeof(u64) * AS_S_WORDS);
    if (e == hipSuccess && cfg->filter && cfg->n_nodes) e = gs_dev_alloc(&h->d_filter, nodes);
    if (e == hipSuccess && cfg->n_nodes) e = hipMemcpyAsync(h->d_known, cfg->known_taxids, sizeof(int32_t) * nodes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && h->d_filter) e = hipMemcpyAsync(h->d_filter, cfg->filter, nodes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        gs_asmsum_destroy(h);
        return hip_fail(e, "gs_asmsum_create");
    }
    if ((rc = as_entry_room(h, std::max<int64_t>(cfg->reserve_entries, 1), std::max<int64_t>(cfg->reserve_entries * 128, 1)))) {
        gs_asmsum_destroy(h);
        return rc;
    }
    *out = h;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_asmsum_get_device(gs_asmsum *h, int *device) try {
    return lines_get_device(h, device);
}
GS_API_CATCH

extern "C" int gs_asmsum_submit(gs_asmsum *h, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]) try {
    int rc = lines_args(h, text, n_bytes, mem, report);
    if (rc) return rc;
    if (h->finished) return fail(GS_E_STATE, "gs_asmsum_submit comes in front of gs_asmsum_finish");
    if (h->host_only) return fail(GS_E_UNSUPPORTED, "a host-only assembly summary handle (device -1) takes entries through gs_asmsum_append alone");
    int64_t n_tiles = 0;
    u64 small[AS_S_COUNTS];
    rc = lines_open(*h, text, n_bytes, mem, report, GS_AS_TILE, 1, GS_AS_NONE, AS_S_COUNTS, &n_tiles);
    if (rc || n_bytes == 0) return rc;
    GsAsmsumParams P{};
    P.text = h->d_text;
    P.n_bytes = n_bytes;
    P.n_tiles = n_tiles;
    P.last = last != 0;
    P.key_field = h->key_field;
    P.quality_mask = h->quality_mask;
    P.reference_only = h->reference_only;
    P.known = h->d_known;
    P.filter = h->d_filter;
    P.n_nodes = h->n_nodes;
    P.tile_lt = (unsigned long long *)h->d_tile;
    P.tile_tail = h->d_tail;
    P.scan_tot = (unsigned long long *)h->d_small + AS_S_SCAN;
    P.status = (uint32_t *)(h->d_small + AS_S_STATUS);
    P.chunk = (unsigned long long *)h->d_small + AS_S_CHUNK;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_asmsum_tiles(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    u64 lines_tabs = 0;
    uint8_t last_byte = 0;
    HIP_TRY(hipMemcpyAsync(&lines_tabs, h->d_small + AS_S_SCAN, sizeof(u64), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&last_byte, h->d_text + n_bytes - 1, 1, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the first wait of a chunk: its lines size the slots
    const int64_t n_lines = (int64_t)(lines_tabs & 0xffffffffull) + (last_byte != '\n');
    const int64_t n_blocks = (n_lines + GS_AS_LINE_BLOCK - 1) / GS_AS_LINE_BLOCK;
    if (h->line_cap < (size_t)n_lines) {
        const size_t cap = (size_t)n_lines + (size_t)n_lines / 4;
        h->line_cap = 0;
        if ((rc = renew(&h->d_slots, cap * GS_AS_SLOT))) return rc;
        if ((rc = renew(&h->d_high, cap))) return rc;
        if ((rc = renew(&h->d_verdict, cap))) return rc;
        h->line_cap = cap;
    }
    if ((rc = grow(&h->d_line_blk, &h->blk_cap, (size_t)n_blocks + 1, h->stream))) return rc;
    HIP_TRY(hipMemsetAsync(h->d_high, 0, (size_t)n_lines, h->stream));
    P.n_lines = n_lines;
    P.slots = h->d_slots;
    P.high = h->d_high;
    P.verdict = (unsigned long long *)h->d_verdict;
    P.line_blk = (unsigned long long *)h->d_line_blk;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_asmsum_judge(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(small, h->d_small, sizeof(small), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the second: its verdict and its counts, in front of the write pass
    if (lines_refused(small[AS_S_STATUS], GS_AS_NONE, report)) return timer_collect(h->timer);
    const int64_t n_put = (int64_t)small[AS_S_CHUNK + GS_AS_C_KEPT], n_pool = (int64_t)small[AS_S_CHUNK + GS_AS_C_POOL];
    report[0] = (int64_t)small[AS_S_CHUNK + GS_AS_C_COUNTED];
    report[1] = n_put;
    report[2] = (int64_t)small[AS_S_CHUNK + GS_AS_C_SHORT];
    report[6] = (int64_t)small[AS_S_CHUNK + GS_AS_C_SKIPPED];
    report[7] = n_pool;
    if (n_put > 0) {
        if ((rc = as_entry_room(h, n_put, n_pool))) return rc;
        if ((rc = grow(&h->d_put_line, &h->put_cap, (size_t)n_put, h->stream))) return rc;
        P.entries = h->d_entries;
        P.first_entry = h->n_entries;
        P.entry_cap = (int64_t)h->entry_cap;
        P.first_line = h->n_lines;
        P.pool = h->d_pool;
        P.pool_used = (unsigned long long)h->pool_used;
        P.pool_cap = (unsigned long long)h->pool_cap;
        P.put_line = h->d_put_line;
        if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
        HIP_TRY(gs_launch_asmsum_write(&P, n_put, h->stream));
        if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->n_entries += n_put;
    h->pool_used += n_pool;
    h->n_counted += report[0];
    h->n_lines += n_lines;
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_asmsum_append(gs_asmsum *h, const int32_t *nodes, const uint8_t *quality, const uint8_t *is_ref, const int64_t *lines,
                                const uint64_t *str_off, const uint8_t *pool, int64_t n, int64_t n_counted, int64_t n_lines) try {
    if (!h) return fail(GS_E_INVALID, "asmsum is NULL");
    if (n < 0 || n_counted < n || n_lines < n_counted) return fail(GS_E_INVALID, "n < 0, n_counted < n or n_lines < n_counted");
    if (n > 0 && (!nodes || !quality || !is_ref || !lines || !str_off)) return fail(GS_E_INVALID, "NULL argument");
    if (h->finished) return fail(GS_E_STATE, "gs_asmsum_append comes in front of gs_asmsum_finish");
    for (int64_t i = 0; i < n; i++) {
        if (nodes[i] < 0 || nodes[i] >= h->n_nodes) return fail(GS_E_INVALID, "a node is no index into known_taxids");
        if (quality[i] < 1 || quality[i] > 10) return fail(GS_E_INVALID, "a quality is an ordinal from 1 to 10");
        if (lines[i] < 0) return fail(GS_E_INVALID, "a line is negative");
        for (int k = 0; k < 3; k++)
            if (str_off[3 * i + k + 1] < str_off[3 * i + k]) return fail(GS_E_INVALID, "str_off must ascend");
        if (str_off[3 * i + 3] == str_off[3 * i + 2]) return fail(GS_E_INVALID, "an entry has an empty ftp path");
    }
    const size_t n_pool = n > 0 ? (size_t)(str_off[3 * n] - str_off[0]) : 0;
    if (n_pool > 0 && !pool) return fail(GS_E_INVALID, "pool is NULL");
    if (n > 0 && h->host_only) {
        for (int64_t i = 0; i < n; i++) {
            gs_host::AsmsumEntry e;
            e.node = nodes[i];
            e.quality = quality[i];
            e.is_ref = is_ref[i] != 0;
            e.line = lines[i];
            const char *s = (const char *)pool;
            e.taxid.assign(s + str_off[3 * i], s + str_off[3 * i + 1]);
            e.species.assign(s + str_off[3 * i + 1], s + str_off[3 * i + 2]);
            e.ftp.assign(s + str_off[3 * i + 2], s + str_off[3 * i + 3]);
            h->store.entries.push_back(std::move(e));
        }
        h->n_entries += n;
    } else if (n > 0) {
        HIP_TRY(hipSetDevice(h->device));
        int rc = as_entry_room(h, n, (int64_t)n_pool);
        if (rc) return rc;
        std::vector<GsAsmEntry> ent((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            GsAsmEntry &e = ent[(size_t)i];
            e.node = nodes[i];
            e.meta = (uint32_t)quality[i] | (is_ref[i] ? 1u << 8 : 0u);
            e.line = lines[i];
            e.pool_off = (unsigned long long)h->pool_used + (str_off[3 * i] - str_off[0]);
            for (int k = 0; k < 3; k++) e.len[k] = (uint32_t)(str_off[3 * i + k + 1] - str_off[3 * i + k]);
            e.pad = 0;
        }
        HIP_TRY(hipMemcpyAsync(h->d_entries + h->n_entries, ent.data(), (size_t)n * sizeof(GsAsmEntry), hipMemcpyHostToDevice, h->stream));
        if (n_pool) HIP_TRY(hipMemcpyAsync(h->d_pool + h->pool_used, pool + str_off[0], n_pool, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->n_entries += n;
        h->pool_used += (int64_t)n_pool;
    }
    h->n_counted += n_counted;
    h->n_lines += n_lines;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_asmsum_finish(gs_asmsum *h, int32_t max_per_node, int64_t info[4]) try {
    if (!h || !info) return fail(GS_E_INVALID, "NULL argument");
    if (h->finished) return fail(GS_E_STATE, "gs_asmsum_finish was called before");
    if (h->host_only) {
        h->store.finish(max_per_node);
        h->n_picked = (int64_t)h->store.picked.size();
        h->nodes_with_entries = h->store.nodes_with_entries;
    } else {
        HIP_TRY(hipSetDevice(h->device));
        const int64_t n = h->n_entries;
        const size_t room = (size_t)std::max<int64_t>(n, 1), words = (size_t)h->n_nodes + 1;
        size_t tmp_bytes = 0;
        HIP_TRY(gs_asmsum_cap_bytes(n, h->n_nodes, &tmp_bytes));
        uint32_t *node_words = nullptr, *seq = nullptr, *perm = nullptr;  // seq | seq_alt
        u64 *key = nullptr, *lens = nullptr;                              // key | key_alt
        void *tmp = nullptr;
        GsAsmEntry *out = nullptr;
        u64 *str_off = nullptr;
        uint8_t *out_pool = nullptr;
        u64 counts[2] = {0, 0}, pool_bytes = 0;
        hipError_t e = gs_dev_alloc(&node_words, 4 * words * sizeof(uint32_t));
        if (e == hipSuccess) e = gs_dev_alloc(&key, 2 * room * sizeof(u64));
        if (e == hipSuccess) e = gs_dev_alloc(&seq, 2 * room * sizeof(uint32_t));
        if (e == hipSuccess) e = gs_dev_alloc(&perm, room * sizeof(uint32_t));
        if (e == hipSuccess) e = gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1));
        int rc = e == hipSuccess ? timer_start(h->timer, h->profile, h->stream) : hip_fail(e, "gs_asmsum_finish");
        if (!rc) {
            e = gs_asmsum_cap(h->d_entries, n, h->n_nodes, max_per_node, node_words, key, key + room, seq, seq + room, tmp, tmp_bytes, perm,
                              (unsigned long long *)h->d_small + AS_S_COUNTS, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(counts, h->d_small + AS_S_COUNTS, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            const size_t m = (size_t)counts[0];
            if (e == hipSuccess) e = gs_dev_alloc(&lens, (3 * m + 1) * sizeof(u64));
            if (e == hipSuccess) e = gs_dev_alloc(&str_off, (3 * m + 1) * sizeof(u64));
            if (e == hipSuccess) e = gs_dev_alloc(&out, std::max<size_t>(m, 1) * sizeof(GsAsmEntry));
            if (e == hipSuccess) e = gs_asmsum_pick_sizes(h->d_entries, perm, (int64_t)m, lens, str_off, tmp, tmp_bytes, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&pool_bytes, str_off + 3 * m, sizeof(u64), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e == hipSuccess) e = gs_dev_alloc(&out_pool, std::max<size_t>((size_t)pool_bytes, 1));
            if (e == hipSuccess) e = gs_asmsum_pick_gather(h->d_entries, perm, (int64_t)m, str_off, h->d_pool, out, out_pool, h->stream);
            if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) rc = hip_fail(e, "gs_asmsum_finish");
        }
        for (void *p : {(void *)node_words, (void *)key, (void *)seq, (void *)perm, (void *)tmp, (void *)lens}) gs_dev_free(p);
        if (rc) {
            for (void *p : {(void *)out, (void *)str_off, (void *)out_pool}) gs_dev_free(p);
            return rc;
        }
        h->d_out = out;
        h->d_str_off = str_off;
        h->d_out_pool = out_pool;
        h->n_picked = (int64_t)counts[0];
        h->nodes_with_entries = (int64_t)counts[1];
        h->out_pool_bytes = (int64_t)pool_bytes;
        gs_dev_free(h->d_entries);  // (the picks stand for them from here on)
        gs_dev_free(h->d_pool);
        h->d_entries = nullptr;
        h->d_pool = nullptr;
        h->entry_cap = h->pool_cap = 0;
        if ((rc = timer_collect(h->timer))) return rc;
    }
    h->finished = true;
    info[0] = h->n_entries;
    info[1] = h->n_picked;
    info[2] = h->nodes_with_entries;
    info[3] = h->n_counted;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_asmsum_fetch(gs_asmsum *h, int32_t *nodes, uint8_t *quality, uint8_t *is_ref, int64_t *lines, uint64_t *str_off, uint8_t *pool) try {
    if (!h) return fail(GS_E_INVALID, "asmsum is NULL");
    if (!h->finished) return fail(GS_E_STATE, "gs_asmsum_fetch comes behind gs_asmsum_finish");
    const int64_t m = h->n_picked;
    if (h->host_only) {
        uint64_t at = 0;
        for (int64_t j = 0; j < m; j++) {
            const gs_host::AsmsumEntry &e = h->store.entries[h->store.picked[(size_t)j]];
            if (nodes) nodes[j] = e.node;
            if (quality) quality[j] = e.quality;
            if (is_ref) is_ref[j] = e.is_ref;
            if (lines) lines[j] = e.line;
            for (const std::string *s : {&e.taxid, &e.species, &e.ftp}) {
                if (str_off) str_off[3 * j + (s == &e.taxid ? 0 : s == &e.species ? 1 : 2)] = at;
                if (pool && !s->empty()) memcpy(pool + at, s->data(), s->size());
                at += s->size();
            }
        }
        if (str_off) str_off[3 * m] = at;
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (m && (nodes || quality || is_ref || lines)) {
        std::vector<GsAsmEntry> ent((size_t)m);
        HIP_TRY(hipMemcpy(ent.data(), h->d_out, (size_t)m * sizeof(GsAsmEntry), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < m; j++) {
            const GsAsmEntry &e = ent[(size_t)j];
            if (nodes) nodes[j] = e.node;
            if (quality) quality[j] = (uint8_t)(e.meta & 0xffu);
            if (is_ref) is_ref[j] = (uint8_t)(e.meta >> 8 & 1u);
            if (lines) lines[j] = e.line;
        }
    }
    if (str_off) HIP_TRY(hipMemcpy(str_off, h->d_str_off, (size_t)(3 * m + 1) * sizeof(u64), hipMemcpyDeviceToHost));
    if (pool && h->out_pool_bytes) HIP_TRY(hipMemcpy(pool, h->d_out_pool, (size_t)h->out_pool_bytes, hipMemcpyDeviceToHost));
    return GS_OK;
}
GS_API_CATCH

extern "C" int64_t gs_asmsum_file_name(const uint8_t *ftp, int64_t n, uint8_t *out, int64_t cap) {
    if (!ftp || n <= 0 || cap < 0 || (cap > 0 && !out)) return fail(GS_E_INVALID, "an ftp path has at least one byte (the reference throws on an empty one)");
    size_t from = 0, to = 0;
    gs_host::asmsum_base_name(ftp, (size_t)n, &from, &to);
    static const char suffix[] = "_genomic.fna.gz";
    const int64_t base = (int64_t)(to - from), len = base + (int64_t)sizeof(suffix) - 1;
    for (int64_t i = 0; i < len && i < cap; i++) out[i] = i < base ? ftp[from + (size_t)i] : (uint8_t)suffix[i - base];
    return len;
}

extern "C" int gs_asmsum_kernel_time(gs_asmsum *h, int profile, int64_t *launches, double *total_ms) try {
    if (!h) return fail(GS_E_INVALID, "asmsum is NULL");
    return lines_kernel_time(*h, h->host_only, profile, launches, total_ms);
}
GS_API_CATCH

// ---------------------------------------------------------------------------------------------------
// taxtree: NCBI nodes.dmp / names.dmp to the arrays of the tree; taxnodes selection; small tree (gs_taxtree.hip, gs_taxparse.h)
// ---------------------------------------------------------------------------------------------------

struct gs_taxtree : LineStage {
    bool host_only = false;  // device == -1
    bool on_host = false;    // the finished tree lives in `tree`: a host-only handle, or a device handle that met duplicate ids
    int state = 0;           // 0: nodes come in; 1: gs_taxtree_finish_nodes has succeeded
    GsTaxRanks *d_ranks = nullptr;
    uint4 *d_slots = nullptr;
    size_t slot_cap = 0;
    int64_t n_slots = 0;
    gs_host::TaxNodesExact nodes;  // the line-by-line reader of nodes; on a host-only handle its slots are the input
    gs_host::TaxNamesExact names;
    gs_host::TaxHostTree tree;     // on_host: all of it; else taxids, names and has_name alone
    // the finished tree on the device
    GsTaxTreeArrays A{};
    int32_t *d_taxids = nullptr;
    int32_t n_reach = 0, max_depth = 0;
    int64_t n_cyc = 0;
    std::vector<uint8_t> h_cyc;  // n_cyc > 0: the nodes on cycles
    // names the device judged (gs_taxtree_submit_names): per node the winning key, and where its name lies in the pool
    u64 *d_win = nullptr, *d_name_off = nullptr;
    uint32_t *d_name_len = nullptr;
    uint8_t *d_pool = nullptr;
    size_t pool_cap = 0;
    double finish_ms[3] = {0, 0, 0};  // the last finish under profile: distinct ids and parents | child order | tree steps
};
// d_small: status | scan sum | counts[6]
enum { TT_S_STATUS = 0, TT_S_SCAN = 1, TT_S_COUNTS = 2, TT_S_WORDS = TT_S_COUNTS + 6 };
static_assert(TT_S_STATUS == 0 && TT_S_COUNTS <= LINES_SMALL_MAX, "the status is the first word of d_small");

static void tt_free_tree(gs_taxtree *h) {
    for (void *p : {(void *)h->d_win, (void *)h->d_name_off, (void *)h->d_name_len, (void *)h->d_pool}) gs_dev_free(p);
    h->d_win = h->d_name_off = nullptr;
    h->d_name_len = nullptr;
    h->d_pool = nullptr;
    h->pool_cap = 0;
    for (void *p : {(void *)h->d_taxids, (void *)h->A.parent, (void *)h->A.rank, (void *)h->A.line_of, (void *)h->A.depth, (void *)h->A.position,
                    (void *)h->A.subtree, (void *)h->A.node_at, (void *)h->A.cyc})
        gs_dev_free(p);
    h->A = GsTaxTreeArrays{};
    h->d_taxids = nullptr;
}

extern "C" int gs_taxtree_destroy(gs_taxtree *h) try {
    if (!h) return GS_OK;
    if (!h->host_only) {
        hipSetDevice(h->device);
        if (h->stream) hipStreamSynchronize(h->stream);
        tt_free_tree(h);
        gs_dev_free(h->d_ranks);
        gs_dev_free(h->d_slots);
        lines_free(*h);
    }
    delete h;
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_create(gs_taxtree **out, int device) try {
    if (!out) return fail(GS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (device < -1) return fail(GS_E_INVALID, "device must be -1 (host only) or a device index");
    int rc = device == -1 ? (int)GS_OK : use_device(device);
    if (rc) return rc;
    gs_taxtree *h = new gs_taxtree();
    h->device = device;
    h->host_only = device == -1;
    if (h->host_only) {
        *out = h;
        return GS_OK;
    }
    GsTaxRanks ranks{};
    for (int r = 0; r < GS_TT_N_RANKS; r++) {
        const size_t len = strlen(gs_host::TAX_RANK_NAMES[r]);
        ranks.len[r] = (uint8_t)len;
        memcpy(ranks.text[r], gs_host::TAX_RANK_NAMES[r], len);
    }
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_ranks, sizeof(GsTaxRanks));
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_small, sizeof(u64) * TT_S_WORDS);
    if (e == hipSuccess) e = hipMemcpyAsync(h->d_ranks, &ranks, sizeof(ranks), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (ranks is a local)
    if (e != hipSuccess) {
        gs_taxtree_destroy(h);
        return hip_fail(e, "gs_taxtree_create");
    }
    *out = h;
    return GS_OK;
}
GS_API_CATCH
static_assert(GS_TT_N_RANKS == gs_host::TAX_N_RANKS, "one list of ranks");

extern "C" int gs_taxtree_get_device(gs_taxtree *h, int *device) try {
    return lines_get_device(h, device);
}
GS_API_CATCH

// room for `need` slots in all; what is there stays
static int tt_slot_room(gs_taxtree *h, size_t need) {
    if (need > h->slot_cap && need > ((size_t)1 << 30)) return fail(GS_E_UNSUPPORTED, "a tree takes at most 2^30 lines");
    return grow_keep(&h->d_slots, &h->slot_cap, (size_t)h->n_slots, need, h->stream, "gs_taxtree: growing the slots");
}

extern "C" int gs_taxtree_submit_nodes(gs_taxtree *h, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]) try {
    int rc = lines_args(h, text, n_bytes, mem, report);
    if (rc) return rc;
    if (h->state != 0) return fail(GS_E_STATE, "gs_taxtree_submit_nodes comes in front of gs_taxtree_finish_nodes");
    if (h->host_only) return fail(GS_E_UNSUPPORTED, "a host-only tree (device -1) takes its lines through gs_taxtree_append_nodes alone");
    int64_t n_tiles = 0;
    u64 small[TT_S_COUNTS];
    rc = lines_open(*h, text, n_bytes, mem, report, GS_TT_TILE, 1, GS_TT_NONE, TT_S_COUNTS, &n_tiles);
    if (rc || n_bytes == 0) return rc;
    GsTaxScanParams P{};
    P.text = h->d_text;
    P.n_bytes = n_bytes;
    P.n_tiles = n_tiles;
    P.last = last != 0;
    P.ranks = h->d_ranks;
    P.tile_lb = (unsigned long long *)h->d_tile;
    P.tile_tail = h->d_tail;
    P.scan_tot = (unsigned long long *)h->d_small + TT_S_SCAN;
    P.status = (uint32_t *)(h->d_small + TT_S_STATUS);
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_taxtree_tiles(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    uint8_t tail = '\n';
    HIP_TRY(hipMemcpyAsync(small, h->d_small, sizeof(small), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&tail, h->d_text + n_bytes - 1, 1, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the lines of the chunk: its slots need room
    const int64_t n_lines = (int64_t)(uint32_t)small[TT_S_SCAN] + (tail != '\n');
    if ((rc = tt_slot_room(h, (size_t)(h->n_slots + n_lines)))) return rc;
    HIP_TRY(hipMemsetAsync(h->d_slots + h->n_slots, 0, (size_t)n_lines * sizeof(uint4), h->stream));
    P.slots = h->d_slots;
    P.first_line = h->n_slots;
    P.slot_cap = h->n_slots + n_lines;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_taxtree_scan(&P, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(small, h->d_small, sizeof(small), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    report[0] = n_lines;
    // (of a refused chunk, what the scan wrote lies behind n_slots: the handle is as it was)
    if (lines_refused(small[TT_S_STATUS], GS_TT_NONE, report)) return timer_collect(h->timer);
    report[2] = n_lines;
    h->n_slots += n_lines;
    h->nodes.line_no += n_lines;
    return timer_collect(h->timer);
}
GS_API_CATCH

static int tt_parse_fail(const gs_host::TaxError &err, const char *what) {
    return fail(err.code == 2 ? GS_E_UNSUPPORTED : GS_E_INVALID, std::string(what) + " line " + std::to_string(err.line) + ": " + err.what);
}

extern "C" int gs_taxtree_append_nodes(gs_taxtree *h, const uint8_t *text, int64_t n_bytes, int last, int64_t report[8]) try {
    if (!h || !report) return fail(GS_E_INVALID, "NULL argument");
    if (n_bytes < 0) return fail(GS_E_INVALID, "n_bytes < 0");
    if (n_bytes > 0 && !text) return fail(GS_E_INVALID, "text is NULL");
    if (h->state != 0) return fail(GS_E_STATE, "gs_taxtree_append_nodes comes in front of gs_taxtree_finish_nodes");
    for (int i = 0; i < 8; i++) report[i] = 0;
    report[4] = -1;
    const int64_t line0 = h->nodes.line_no;
    const size_t before = h->nodes.slots.size();
    if (!h->nodes.feed(text, (size_t)n_bytes, last != 0)) {
        h->nodes.slots.resize(before);
        const gs_host::TaxError err = h->nodes.err;
        h->nodes.line_no = line0;
        return tt_parse_fail(err, "nodes");
    }
    report[0] = h->nodes.line_no - line0;
    report[2] = (int64_t)(h->nodes.slots.size() - before);
    if (h->host_only) {
        h->n_slots = (int64_t)h->nodes.slots.size();
        return GS_OK;
    }
    const size_t n = h->nodes.slots.size();
    if (n) {
        HIP_TRY(hipSetDevice(h->device));
        int rc = tt_slot_room(h, (size_t)h->n_slots + n);
        if (rc) return rc;
        static_assert(sizeof(gs_host::TaxSlot) == sizeof(uint4), "a slot is 16 bytes on both sides");
        HIP_TRY(hipMemcpyAsync(h->d_slots + h->n_slots, h->nodes.slots.data(), n * sizeof(uint4), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->n_slots += (int64_t)n;
        h->nodes.slots.clear();
    }
    return GS_OK;
}
GS_API_CATCH

// info: [0] nodes, [1] nodes the root reaches, [2] the deepest of them, [3] lines whose id had a line before, [4] 1: the tree
// lives on the host, [5] nodes on a cycle of parent links, [6] slots
static int tt_finish_host(gs_taxtree *h, const gs_host::TaxSlot *slots, size_t m, int64_t info[8]) {
    std::string why;
    if (!h->tree.build(slots, m, &why)) return fail(GS_E_INVALID, "gs_taxtree_finish_nodes: " + why);
    h->on_host = true;
    h->state = 1;
    h->n_reach = 0;
    h->max_depth = 0;
    for (int32_t v = 0; v < h->tree.n; v++) {
        h->n_reach += h->tree.position[(size_t)v] >= 0;
        h->max_depth = std::max(h->max_depth, h->tree.depth[(size_t)v]);
    }
    info[0] = h->tree.n;
    info[1] = h->n_reach;
    info[2] = h->max_depth;
    info[3] = h->tree.duplicates;
    info[4] = 1;
    info[6] = (int64_t)m;
    return GS_OK;
}

extern "C" int gs_taxtree_finish_nodes(gs_taxtree *h, int64_t info[8]) try {
    if (!h || !info) return fail(GS_E_INVALID, "NULL argument");
    if (h->state != 0) return fail(GS_E_STATE, "gs_taxtree_finish_nodes was called before");
    for (int i = 0; i < 8; i++) info[i] = 0;
    if (h->host_only) return tt_finish_host(h, h->nodes.slots.data(), h->nodes.slots.size(), info);
    const int64_t m = h->n_slots;
    if (m == 0) return fail(GS_E_INVALID, "gs_taxtree_finish_nodes: no root: no line has the id 1 and the parent 1");
    HIP_TRY(hipSetDevice(h->device));
    u64 *counts_d = h->d_small + TT_S_COUNTS;
    u64 counts[6] = {};
    HIP_TRY(hipMemcpy(counts_d, counts, sizeof(counts), hipMemcpyHostToDevice));  // (the stream is idle between calls)
    size_t tmp_bytes = 0;
    HIP_TRY(gs_taxtree_sort_bytes(2 * m, &tmp_bytes));
    // one block of scratch for every step: [0, 8m) words for the distinct step, reused by the steps behind it
    uint32_t *w = nullptr;
    void *tmp = nullptr;
    int rc = GS_OK;
    hipError_t e = gs_dev_alloc(&w, (size_t)8 * (size_t)m * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1));
    if (e == hipSuccess) e = gs_dev_alloc(&h->d_taxids, (size_t)2 * (size_t)m * sizeof(int32_t));
    const size_t pair0 = h->timer.pending.size();
    std::vector<int> phase_of;  // of the event pairs from pair0 on
    auto timed = [&](int phase, bool begin) {
        if (!begin && h->profile) phase_of.push_back(phase);
        return begin ? timer_start(h->timer, h->profile, h->stream) : timer_stop(h->timer, h->profile, h->stream);
    };
    auto bail = [&](int code) {
        hipStreamSynchronize(h->stream);
        timer_collect(h->timer);  // (the pairs handed in so far; an open one is taken up by the next start)
        gs_dev_free(w);
        gs_dev_free(tmp);
        tt_free_tree(h);
        return code;
    };
    if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes"));
    if ((rc = timed(0, true))) return bail(rc);
    e = gs_taxtree_distinct(h->d_slots, m, w, w + 2 * m, w + 4 * m, w + 6 * m, tmp, tmp_bytes, h->d_taxids, (unsigned long long *)counts_d, h->stream);
    if (e == hipSuccess && (rc = timed(0, false))) return bail(rc);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, counts_d, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes: distinct ids"));
    const int64_t n = (int64_t)(uint32_t)counts[4] + (int64_t)(counts[4] >> 32);
    if (n <= 0) return bail(fail(GS_E_INVALID, "gs_taxtree_finish_nodes: no root: no line has the id 1 and the parent 1"));
    gs_dev_free(w);
    w = nullptr;
    {  // the sorts and scans of n <= 2m nodes: what they ask for, should that be more than what 2m keys asked for
        size_t again = 0;
        e = gs_taxtree_sort_bytes(n, &again);
        if (e == hipSuccess && again > tmp_bytes) {
            gs_dev_free(tmp);
            tmp = nullptr;
            tmp_bytes = again;
            e = gs_dev_alloc(&tmp, tmp_bytes);
        }
        if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes"));
    }
    GsTaxTreeArrays &A = h->A;
    A.n = (int32_t)n;
    A.root = 0;  // ids are positive and ascending: the node "1" is the first or is not there
    A.taxids = h->d_taxids;
    for (int32_t **p : {&A.parent, &A.rank, &A.line_of, &A.depth, &A.position, &A.subtree, &A.node_at})
        if (e == hipSuccess) e = gs_dev_alloc(p, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = gs_dev_alloc(&A.cyc, (size_t)n);
    // scratch of the tree steps, in words: key 2n | key_alt 2n | ord n | ord_alt n | first_child n | next_sib n |
    // succ 2n+2 | succ_alt 2n+2 | val 4n+4 | val_alt 4n+4 | up n | up_alt n
    const size_t N = (size_t)n;
    if (e == hipSuccess) e = gs_dev_alloc(&w, (22 * N + 16) * sizeof(uint32_t));
    if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes"));
    if ((rc = timed(0, true))) return bail(rc);
    e = gs_taxtree_resolve(h->d_slots, m, &A, (unsigned long long *)counts_d, h->stream);
    if (e == hipSuccess && (rc = timed(0, false))) return bail(rc);
    int32_t first[3] = {0, 0, 0};  // taxids[0], parent[0], line_of[0]
    if (e == hipSuccess) e = hipMemcpyAsync(counts, counts_d, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&first[0], h->d_taxids, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&first[1], A.parent, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&first[2], A.line_of, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes: resolve"));
    if (counts[0] > 0) {
        // two lines with one id: the reference lists the node twice and keeps its last parent.  The host's child lists say that.
        std::vector<gs_host::TaxSlot> slots((size_t)m);
        e = hipMemcpy(slots.data(), h->d_slots, (size_t)m * sizeof(uint4), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes: slots to the host"));
        bail(0);
        gs_dev_free(h->d_slots);  // (the tree lives on the host from here on)
        h->d_slots = nullptr;
        h->slot_cap = 0;
        return tt_finish_host(h, slots.data(), slots.size(), info);
    }
    if (first[0] != 1 || first[1] != -1 || first[2] < 0)
        return bail(fail(GS_E_INVALID, "gs_taxtree_finish_nodes: no root: no line has the id 1 and the parent 1"));
    u64 *key = (u64 *)w;
    uint32_t *ord = w + 4 * N, *succ = w + 8 * N;
    int32_t *first_child = (int32_t *)(w + 6 * N), *next_sib = (int32_t *)(w + 7 * N);
    u64 *val = (u64 *)(w + 8 * N + 2 * (2 * N + 2));  // (8N + 4N + 4 words in front: a multiple of two)
    int32_t *up = (int32_t *)(w + 8 * N + 2 * (2 * N + 2) + 4 * (2 * N + 2));
    if ((rc = timed(1, true))) return bail(rc);
    e = gs_taxtree_children(&A, key, key + N, ord, ord + N, tmp, tmp_bytes, first_child, next_sib, h->stream);
    if (e == hipSuccess && (rc = timed(1, false))) return bail(rc);
    if (e == hipSuccess && (rc = timed(2, true))) return bail(rc);
    if (e == hipSuccess) e = gs_taxtree_place(&A, first_child, next_sib, succ, succ + 2 * N + 2, val, val + 2 * N + 2, up, up + N, (unsigned long long *)counts_d, h->stream);
    if (e == hipSuccess) rc = timed(2, false);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, counts_d, sizeof(counts), hipMemcpyDeviceToHost, h->stream);
    h->tree.taxids.resize(N);
    if (e == hipSuccess) e = hipMemcpyAsync(h->tree.taxids.data(), h->d_taxids, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes: tree steps"));
    if (rc) return bail(rc);
    h->finish_ms[0] = h->finish_ms[1] = h->finish_ms[2] = 0;
    for (size_t i = 0; i < phase_of.size() && pair0 + i < h->timer.pending.size(); i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, h->timer.pending[pair0 + i].first, h->timer.pending[pair0 + i].second) == hipSuccess) h->finish_ms[phase_of[i]] += ms;
    }
    h->n_reach = (int32_t)counts[1];
    h->max_depth = (int32_t)counts[2];
    h->n_cyc = 0;
    if (counts[3] > 0) {
        h->h_cyc.resize(N);
        e = hipMemcpy(h->h_cyc.data(), A.cyc, N, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return bail(hip_fail(e, "gs_taxtree_finish_nodes: cycle flags"));
        for (uint8_t c : h->h_cyc) h->n_cyc += c;
    }
    gs_dev_free(w);
    gs_dev_free(tmp);
    gs_dev_free(h->d_slots);
    h->d_slots = nullptr;
    h->slot_cap = 0;
    h->tree.n = A.n;
    h->tree.names.assign(N, std::string());
    h->tree.has_name.assign(N, 0);
    h->tree.name_key.assign(N, 0);
    h->state = 1;
    info[0] = n;
    info[1] = h->n_reach;
    info[2] = h->max_depth;
    info[5] = h->n_cyc;
    info[6] = m;
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_taxtree_submit_names(gs_taxtree *h, const uint8_t *text, int64_t n_bytes, int mem, int last, int64_t report[8]) try {
    int rc = lines_args(h, text, n_bytes, mem, report);
    if (rc) return rc;
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_submit_names comes behind gs_taxtree_finish_nodes");
    if (h->on_host) return fail(GS_E_UNSUPPORTED, "the tree lives on the host (device -1, or duplicate ids): names go through gs_taxtree_append_names");
    int64_t n_tiles = 0;
    u64 small[TT_S_COUNTS];
    rc = lines_open(*h, text, n_bytes, mem, report, GS_TT_TILE, 1, GS_TT_NONE, TT_S_COUNTS, &n_tiles);
    if (rc || n_bytes == 0) return rc;
    const size_t N = (size_t)h->tree.n;
    u64 *pool_used_d = h->d_small + TT_S_COUNTS + 5;
    if (!h->d_win) {  // the first chunk of names
        hipError_t e = gs_dev_alloc(&h->d_win, N * sizeof(u64));
        if (e == hipSuccess) e = gs_dev_alloc(&h->d_name_off, N * sizeof(u64));
        if (e == hipSuccess) e = gs_dev_alloc(&h->d_name_len, N * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemsetAsync(h->d_win, 0, N * sizeof(u64), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(pool_used_d, 0, sizeof(u64), h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            gs_dev_free(h->d_win);
            h->d_win = nullptr;
            return hip_fail(e, "gs_taxtree_submit_names");
        }
    }
    GsTaxScanParams P{};
    P.text = h->d_text;
    P.n_bytes = n_bytes;
    P.n_tiles = n_tiles;
    P.last = last != 0;
    P.tile_lb = (unsigned long long *)h->d_tile;
    P.tile_tail = h->d_tail;
    P.scan_tot = (unsigned long long *)h->d_small + TT_S_SCAN;
    P.status = (uint32_t *)(h->d_small + TT_S_STATUS);
    P.first_line = h->names.line_no;
    P.taxids = h->d_taxids;
    P.n_nodes = h->tree.n;
    P.win = (unsigned long long *)h->d_win;
    P.name_off = (unsigned long long *)h->d_name_off;
    P.name_len = h->d_name_len;
    P.pool_used = (unsigned long long *)pool_used_d;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_taxtree_tiles(&P, h->stream));
    HIP_TRY(gs_launch_taxtree_names(&P, 0, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    uint8_t tail = '\n';
    u64 used = 0;
    HIP_TRY(hipMemcpyAsync(small, h->d_small, sizeof(small), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&tail, h->d_text + n_bytes - 1, 1, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&used, pool_used_d, sizeof(used), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));  // the one wait of a chunk: its verdict
    const int64_t n_lines = (int64_t)(uint32_t)small[TT_S_SCAN] + (tail != '\n');
    report[0] = n_lines;
    if (lines_refused(small[TT_S_STATUS], GS_TT_NONE, report)) return timer_collect(h->timer);  // (nothing was written: the handle is as it was)
    // every name of the chunk has room, whoever wins; what the pool holds stays
    const size_t need = (size_t)used + (size_t)n_bytes;
    if ((rc = grow_keep(&h->d_pool, &h->pool_cap, (size_t)used, need, h->stream, "gs_taxtree_submit_names: growing the pool"))) return rc;
    P.pool = h->d_pool;
    if ((rc = timer_start(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(gs_launch_taxtree_names(&P, 1, h->stream));
    HIP_TRY(gs_launch_taxtree_names(&P, 2, h->stream));
    if ((rc = timer_stop(h->timer, h->profile, h->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    report[2] = n_lines;
    h->names.line_no += n_lines;
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_taxtree_append_names(gs_taxtree *h, const uint8_t *text, int64_t n_bytes, int last) try {
    if (!h) return fail(GS_E_INVALID, "tree is NULL");
    if (n_bytes < 0) return fail(GS_E_INVALID, "n_bytes < 0");
    if (n_bytes > 0 && !text) return fail(GS_E_INVALID, "text is NULL");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_append_names comes behind gs_taxtree_finish_nodes");
    if (!h->names.feed(h->tree, text, (size_t)n_bytes, last != 0)) return tt_parse_fail(h->names.err, "names");
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_fetch(gs_taxtree *h, int32_t *taxids, int32_t *parent, int32_t *depth, int32_t *position, int32_t *subtree, int32_t *rank) try {
    if (!h) return fail(GS_E_INVALID, "tree is NULL");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_fetch comes behind gs_taxtree_finish_nodes");
    const size_t bytes = (size_t)h->tree.n * sizeof(int32_t);
    if (taxids) memcpy(taxids, h->tree.taxids.data(), bytes);
    if (h->on_host) {
        if (parent) memcpy(parent, h->tree.parent.data(), bytes);
        if (depth) memcpy(depth, h->tree.depth.data(), bytes);
        if (position) memcpy(position, h->tree.position.data(), bytes);
        if (subtree) memcpy(subtree, h->tree.subtree.data(), bytes);
        if (rank) memcpy(rank, h->tree.rank.data(), bytes);
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (parent) HIP_TRY(hipMemcpy(parent, h->A.parent, bytes, hipMemcpyDeviceToHost));
    if (depth) HIP_TRY(hipMemcpy(depth, h->A.depth, bytes, hipMemcpyDeviceToHost));
    if (position) HIP_TRY(hipMemcpy(position, h->A.position, bytes, hipMemcpyDeviceToHost));
    if (subtree) HIP_TRY(hipMemcpy(subtree, h->A.subtree, bytes, hipMemcpyDeviceToHost));
    if (rank) HIP_TRY(hipMemcpy(rank, h->A.rank, bytes, hipMemcpyDeviceToHost));
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_fetch_names(gs_taxtree *h, int64_t *offsets, uint8_t *bytes, int64_t cap) try {
    if (!h || !offsets) return fail(GS_E_INVALID, "NULL argument");
    if (cap < 0) return fail(GS_E_INVALID, "cap < 0");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_fetch_names comes behind gs_taxtree_finish_nodes");
    if (h->d_win) {  // what the device judged joins what the host judged: per node the higher key has the name
        HIP_TRY(hipSetDevice(h->device));
        const size_t N = (size_t)h->tree.n;
        std::vector<u64> win(N), off(N);
        std::vector<uint32_t> len(N);
        u64 used = 0;
        HIP_TRY(hipMemcpy(win.data(), h->d_win, N * sizeof(u64), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(off.data(), h->d_name_off, N * sizeof(u64), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(len.data(), h->d_name_len, N * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&used, h->d_small + TT_S_COUNTS + 5, sizeof(used), hipMemcpyDeviceToHost));
        std::vector<uint8_t> pool((size_t)used + 1);
        if (used) HIP_TRY(hipMemcpy(pool.data(), h->d_pool, (size_t)used, hipMemcpyDeviceToHost));
        for (size_t v = 0; v < N; v++)
            if (win[v] > h->tree.name_key[v]) {
                if (off[v] + len[v] > used) return fail(GS_E_HIP, "gs_taxtree_fetch_names: a name lies outside the pool");
                h->tree.names[v].assign((const char *)pool.data() + off[v], len[v]);
                h->tree.has_name[v] = 1;
                h->tree.name_key[v] = win[v];
            }
    }
    int64_t at = 0;
    for (int32_t v = 0; v < h->tree.n; v++) {
        offsets[v] = h->tree.has_name[(size_t)v] ? at : -1 - at;  // (a node without a name: -1 - where the next one starts)
        at += (int64_t)h->tree.names[(size_t)v].size();
    }
    offsets[h->tree.n] = at;
    if (!bytes) return GS_OK;
    if (cap < at) return fail(GS_E_INVALID, "bytes is too small: offsets[n_nodes] says what it takes");
    at = 0;
    for (int32_t v = 0; v < h->tree.n; v++) {
        memcpy(bytes + at, h->tree.names[(size_t)v].data(), h->tree.names[(size_t)v].size());
        at += (int64_t)h->tree.names[(size_t)v].size();
    }
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_select(gs_taxtree *h, const int32_t *requested, int64_t n_requested, const int32_t *excluded, int64_t n_excluded, int cut_rank,
                                 uint8_t *out, int64_t *count) try {
    if (!h || !out) return fail(GS_E_INVALID, "NULL argument");
    if (n_requested < 0 || n_excluded < 0 || (n_requested > 0 && !requested) || (n_excluded > 0 && !excluded))
        return fail(GS_E_INVALID, "a list is NULL or its length negative");
    if (cut_rank < -1 || cut_rank >= GS_TT_N_RANKS) return fail(GS_E_INVALID, "cut_rank is -1 (none) or the ordinal of a rank");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_select comes behind gs_taxtree_finish_nodes");
    const int32_t n = h->tree.n;
    for (int k = 0; k < 2; k++)
        for (int64_t i = 0; i < (k ? n_excluded : n_requested); i++) {
            const int32_t v = (k ? excluded : requested)[i];
            if (v < 0 || v >= n) return fail(GS_E_INVALID, "a requested or excluded node is no index into the tree");
            if (!h->on_host && h->n_cyc && h->h_cyc[(size_t)v])
                return fail(GS_E_INVALID, "a requested or excluded node lies on a cycle of parent links: the reference's descent does not end");
        }
    if (h->on_host) {
        if (!h->tree.select(requested, n_requested, excluded, n_excluded, cut_rank, out))
            return fail(GS_E_INVALID, "a requested or excluded node reaches a cycle: the reference's descent does not end");
        if (count) {
            *count = 0;
            for (int32_t v = 0; v < n; v++) *count += out[v];
        }
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t N = (size_t)n, n_list = (size_t)(n_requested + n_excluded);
    uint8_t *bytes = nullptr;  // marks n | out n
    int32_t *words = nullptr;  // anc 3n | requested | excluded
    hipError_t e = gs_dev_alloc(&bytes, 2 * N);
    if (e == hipSuccess) e = gs_dev_alloc(&words, (3 * N + n_list + 1) * sizeof(int32_t));
    int32_t *d_req = words + 3 * N, *d_exc = d_req + n_requested;
    u64 *d_count = h->d_small + TT_S_COUNTS;
    u64 c = 0;
    if (e == hipSuccess && n_requested) e = hipMemcpyAsync(d_req, requested, (size_t)n_requested * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && n_excluded) e = hipMemcpyAsync(d_exc, excluded, (size_t)n_excluded * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpy(d_count, &c, sizeof(c), hipMemcpyHostToDevice);  // (the stream is idle between calls)
    int rc = e == hipSuccess ? timer_start(h->timer, h->profile, h->stream) : hip_fail(e, "gs_taxtree_select");
    if (!rc) {
        e = gs_launch_taxtree_select(&h->A, d_req, n_requested, d_exc, n_excluded, cut_rank, bytes, words, bytes + N, (unsigned long long *)d_count, h->stream);
        if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out, bytes + N, N, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&c, d_count, sizeof(c), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = hip_fail(e, "gs_taxtree_select");
    }
    e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "gs_taxtree_select");
    gs_dev_free(bytes);
    gs_dev_free(words);
    if (rc) return rc;
    if (count) *count = (int64_t)c;
    return timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_taxtree_small(gs_taxtree *h, const void *flagged, int flag_bytes, int mem, int32_t *n_small, int32_t *node_of_vi, int32_t *parent_vi,
                                int32_t *depth, int32_t *position) try {
    if (!h || !flagged || !n_small) return fail(GS_E_INVALID, "NULL argument");
    if (flag_bytes != 1 && flag_bytes != 4) return fail(GS_E_INVALID, "flag_bytes is 1 (uint8) or 4 (int32, > 0 means flagged)");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_small comes behind gs_taxtree_finish_nodes");
    if (h->host_only && mem != GS_MEM_HOST) return fail(GS_E_UNSUPPORTED, "a host-only tree reads host memory alone");
    const int32_t n = h->tree.n;
    const size_t N = (size_t)n;
    if (h->on_host) {
        std::vector<uint8_t> f8;
        std::vector<int32_t> f32;
        const void *f = flagged;
        if (mem == GS_MEM_DEVICE) {
            HIP_TRY(hipSetDevice(h->device));
            if (flag_bytes == 1) {
                f8.resize(N);
                f = f8.data();
            } else {
                f32.resize(N);
                f = f32.data();
            }
            HIP_TRY(hipMemcpy(const_cast<void *>(f), flagged, N * (size_t)flag_bytes, hipMemcpyDeviceToHost));
        }
        std::vector<int32_t> nodes, parents;
        if (flag_bytes == 1)
            h->tree.small((const uint8_t *)f, nodes, parents);
        else
            h->tree.small((const int32_t *)f, nodes, parents);
        *n_small = (int32_t)nodes.size();
        for (size_t i = 0; i < nodes.size(); i++) {
            if (node_of_vi) node_of_vi[i] = nodes[i];
            if (parent_vi) parent_vi[i] = parents[i];
            if (depth) depth[i] = h->tree.depth[(size_t)nodes[i]];
            if (position) position[i] = h->tree.position[(size_t)nodes[i]];
        }
        return GS_OK;
    }
    HIP_TRY(hipSetDevice(h->device));
    const size_t R = (size_t)h->n_reach;
    size_t tmp_bytes = 0;
    HIP_TRY(gs_taxtree_sort_bytes((int64_t)R, &tmp_bytes));
    uint32_t *w = nullptr;  // pre | sum | req | vi | node_of_vi | parent_vi | depth | position, R words each; then the flags
    void *tmp = nullptr;
    const size_t flag_words = mem == GS_MEM_HOST ? (N * (size_t)flag_bytes + 3) / 4 : 0;
    hipError_t e = gs_dev_alloc(&w, (8 * R + flag_words + 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1));
    const void *d_flag = flagged;
    if (e == hipSuccess && mem == GS_MEM_HOST) {
        e = hipMemcpyAsync(w + 8 * R, flagged, N * (size_t)flag_bytes, hipMemcpyHostToDevice, h->stream);
        d_flag = w + 8 * R;
    }
    int rc = e == hipSuccess ? timer_start(h->timer, h->profile, h->stream) : hip_fail(e, "gs_taxtree_small");
    uint32_t last[2] = {0, 0};
    if (!rc) {
        e = gs_launch_taxtree_small(&h->A, h->n_reach, flag_bytes == 1 ? (const uint8_t *)d_flag : nullptr, flag_bytes == 4 ? (const int32_t *)d_flag : nullptr, w,
                                    w + R, w + 2 * R, w + 3 * R, tmp, tmp_bytes, (int32_t *)(w + 4 * R), (int32_t *)(w + 5 * R), (int32_t *)(w + 6 * R),
                                    (int32_t *)(w + 7 * R), h->stream);
        if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&last[0], w + 3 * R - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);  // req[R - 1]
        if (e == hipSuccess) e = hipMemcpyAsync(&last[1], w + 4 * R - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);  // vi[R - 1]
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        const size_t S = (size_t)last[0] + last[1];
        *n_small = (int32_t)S;
        if (e == hipSuccess && node_of_vi) e = hipMemcpyAsync(node_of_vi, w + 4 * R, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && parent_vi) e = hipMemcpyAsync(parent_vi, w + 5 * R, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && depth) e = hipMemcpyAsync(depth, w + 6 * R, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && position) e = hipMemcpyAsync(position, w + 7 * R, S * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) rc = hip_fail(e, "gs_taxtree_small");
    }
    e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "gs_taxtree_small");
    gs_dev_free(w);
    gs_dev_free(tmp);
    return rc ? rc : timer_collect(h->timer);
}
GS_API_CATCH

extern "C" int gs_taxtree_regions_below(gs_taxtree *h, const int32_t *regions, int mem, const int32_t *selected, int64_t n_selected, int32_t limit,
                                        int check_rank, int32_t *inclusive, int32_t *below, int64_t *n_below) try {
    if (!h || !regions) return fail(GS_E_INVALID, "NULL argument");
    if (n_selected < 0 || (n_selected > 0 && !selected)) return fail(GS_E_INVALID, "the selection is NULL or its length negative");
    if (check_rank < -1 || check_rank >= GS_TT_N_RANKS) return fail(GS_E_INVALID, "check_rank is -1 (any) or the ordinal of a rank");
    if (mem != GS_MEM_HOST && mem != GS_MEM_DEVICE) return fail(GS_E_INVALID, "mem must be GS_MEM_HOST or GS_MEM_DEVICE");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_regions_below comes behind gs_taxtree_finish_nodes");
    if (h->host_only && mem != GS_MEM_HOST) return fail(GS_E_UNSUPPORTED, "a host-only tree reads host memory alone");
    const int32_t n = h->tree.n;
    const size_t N = (size_t)n;
    for (int64_t i = 0; i < n_selected; i++)
        if (selected[i] < 0 || selected[i] >= n) return fail(GS_E_INVALID, "a selected node is no index into the tree");
    if (mem == GS_MEM_HOST)
        for (size_t v = 0; v < N; v++)
            if (regions[v] < 0) return fail(GS_E_INVALID, "a region count is negative");
    const char *cycle = "gs_taxtree_regions_below: a node with regions stands on or below a cycle of parent links: the reference's walk does not end";
    std::vector<int32_t> incl(N), out;
    if (h->on_host) {
        if (mem == GS_MEM_DEVICE) {
            HIP_TRY(hipSetDevice(h->device));
            HIP_TRY(hipMemcpy(incl.data(), regions, N * sizeof(int32_t), hipMemcpyDeviceToHost));
        } else {
            memcpy(incl.data(), regions, N * sizeof(int32_t));
        }
        const std::vector<int32_t> own(incl);
        if (!gs_host::tax_regions_up(h->tree.parent.data(), n, own.data(), nullptr, incl.data())) return fail(GS_E_INVALID, cycle);
        gs_host::tax_regions_below(incl.data(), h->tree.rank.data(), n, selected, n_selected, limit, check_rank, out);
    } else {
        HIP_TRY(hipSetDevice(h->device));
        const size_t R = (size_t)h->n_reach, S = (size_t)n_selected;
        size_t tmp_bytes = 0;
        HIP_TRY(gs_taxtree_sort_bytes((int64_t)N, &tmp_bytes));
        uint32_t *w = nullptr;  // pre R | sum R | incl N | flag N | idx N | out N | selected | regions, if they come from the host
        uint8_t *marks = nullptr;
        void *tmp = nullptr;
        hipError_t e = gs_dev_alloc(&w, (2 * R + 4 * N + S + (mem == GS_MEM_HOST ? N : 0) + 1) * sizeof(uint32_t));
        if (e == hipSuccess) e = gs_dev_alloc(&marks, N);
        if (e == hipSuccess) e = gs_dev_alloc(&tmp, std::max<size_t>(tmp_bytes, 1));
        int32_t *d_incl = (int32_t *)(w + 2 * R), *d_out = (int32_t *)(w + 2 * R + 3 * N), *d_sel = d_out + N;
        uint32_t *d_flag = w + 2 * R + N, *d_idx = d_flag + N;
        const int32_t *d_regions = regions;
        if (e == hipSuccess && mem == GS_MEM_HOST) {
            e = hipMemcpyAsync(d_sel + S, regions, N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
            d_regions = d_sel + S;
        }
        if (e == hipSuccess && S) e = hipMemcpyAsync(d_sel, selected, S * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
        int rc = e == hipSuccess ? timer_start(h->timer, h->profile, h->stream) : hip_fail(e, "gs_taxtree_regions_below");
        if (!rc) {
            e = gs_launch_taxtree_regions(&h->A, h->n_reach, d_regions, w, w + R, tmp, tmp_bytes, d_incl, h->stream);
            if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
            if (e != hipSuccess) rc = hip_fail(e, "gs_taxtree_regions_below");
        }
        if (!rc && R < N) {  // what the root does not reach: the parent walk, on the host
            std::vector<int32_t> parent(N), position(N);
            e = hipMemcpyAsync(incl.data(), d_incl, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(parent.data(), h->A.parent, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(position.data(), h->A.position, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) {
                rc = hip_fail(e, "gs_taxtree_regions_below");
            } else {
                const std::vector<int32_t> own(incl);
                if (!gs_host::tax_regions_up(parent.data(), n, own.data(), position.data(), incl.data())) rc = fail(GS_E_INVALID, cycle);
            }
            if (!rc) {
                e = hipMemcpyAsync(d_incl, incl.data(), N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream);
                if (e != hipSuccess) rc = hip_fail(e, "gs_taxtree_regions_below");
            }
        }
        uint32_t last[2] = {0, 0};
        if (!rc) rc = timer_start(h->timer, h->profile, h->stream);
        if (!rc) {
            e = gs_launch_taxtree_below(&h->A, d_sel, n_selected, d_incl, limit, check_rank, marks, d_flag, d_idx, tmp, tmp_bytes, d_out, h->stream);
            if (e == hipSuccess) rc = timer_stop(h->timer, h->profile, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&last[0], d_flag + N - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&last[1], d_idx + N - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess && inclusive && R == N) e = hipMemcpyAsync(incl.data(), d_incl, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            out.resize((size_t)last[0] + last[1]);
            if (e == hipSuccess && !out.empty()) e = hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
            if (e != hipSuccess) rc = hip_fail(e, "gs_taxtree_regions_below");
        }
        e = hipStreamSynchronize(h->stream);
        if (!rc && e != hipSuccess) rc = hip_fail(e, "gs_taxtree_regions_below");
        gs_dev_free(w);
        gs_dev_free(marks);
        gs_dev_free(tmp);
        if (!rc) rc = timer_collect(h->timer);
        if (rc) return rc;
    }
    if (inclusive) memcpy(inclusive, incl.data(), N * sizeof(int32_t));
    if (below && !out.empty()) memcpy(below, out.data(), out.size() * sizeof(int32_t));
    if (n_below) *n_below = (int64_t)out.size();
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_finish_times(gs_taxtree *h, double ms[3]) try {
    if (!h || !ms) return fail(GS_E_INVALID, "NULL argument");
    if (h->state != 1) return fail(GS_E_STATE, "gs_taxtree_finish_times comes behind gs_taxtree_finish_nodes");
    for (int i = 0; i < 3; i++) ms[i] = h->finish_ms[i];
    return GS_OK;
}
GS_API_CATCH

extern "C" int gs_taxtree_kernel_time(gs_taxtree *h, int profile, int64_t *launches, double *total_ms) try {
    if (!h) return fail(GS_E_INVALID, "tree is NULL");
    return lines_kernel_time(*h, h->host_only, profile, launches, total_ms);
}
GS_API_CATCH

extern "C" int gs_taxtree_read_taxids(const uint8_t *text, int64_t n_bytes, int32_t *requested, int64_t *n_requested, int32_t *excluded, int64_t *n_excluded,
                                      int64_t cap) try {
    if (!n_requested || !n_excluded || n_bytes < 0 || cap < 0 || (n_bytes > 0 && !text)) return fail(GS_E_INVALID, "NULL or negative argument");
    std::vector<int32_t> req, exc;
    gs_host::tax_read_taxids(text, (size_t)n_bytes, req, exc);
    *n_requested = (int64_t)req.size();
    *n_excluded = (int64_t)exc.size();
    if (requested && (int64_t)req.size() <= cap) memcpy(requested, req.data(), req.size() * sizeof(int32_t));
    if (excluded && (int64_t)exc.size() <= cap) memcpy(excluded, exc.data(), exc.size() * sizeof(int32_t));
    return GS_OK;
}
GS_API_CATCH
