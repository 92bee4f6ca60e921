// gs_host.cpp -- C++ host layer above the C ABI (include/gshost.h): the runMatcher / runFilter file pipelines -- raw
// text blocks to the device where the file allows it (TextJob), the reference-exact parser otherwise and as the
// fallback -- with the Kraken-style and filtered-FASTQ writers.  The byte-level side (readers, parser, gzip decoder)
// is in gs_ingest.h / gs_inflate.h, the cut of reader blocks into chunks of whole records in gs_chunk.h, the CSV report
// in gs_report.cpp.  Plain C++17 + zlib; all GPU work goes through the C ABI of include/gsgpu.h.
#include "gs_ingest.h"
#include "gs_chunk.h"
#include "gs_krakenparse.h"
#include "gs_genomeparse.h"
#include "gs_accmapparse.h"
#include "gs_asmsumparse.h"

#include "gs_control.h"

#include <cstddef>
#include <map>

using namespace gs_host;

// ---------------------------------------------------------------------------------------------------
// progress and cancellation (include/gshost.h: gs_host_control_*)
// ---------------------------------------------------------------------------------------------------
static_assert(sizeof(gs_host_progress) == sizeof(gs_control::Record) && offsetof(gs_host_progress, file_reads) == offsetof(gs_control::Record, file_reads) &&
                  offsetof(gs_host_progress, seconds_total) == offsetof(gs_control::Record, seconds_total),
              "gs_host_progress and gs_control::Record are one layout");

struct gs_host_control {
    gs_host_progress_fn fn;
    void *user;
    gs_control::Control ctl;
    static int call(void *self, const gs_control::Record *r) {
        gs_host_control *h = static_cast<gs_host_control *>(self);
        gs_host_progress p;
        memcpy(&p, r, sizeof p);
        return h->fn(h->user, &p);
    }
    gs_host_control(gs_host_progress_fn f, void *u, int32_t every_ms) : fn(f), user(u), ctl(f ? &gs_host_control::call : nullptr, this, every_ms) {}
};

namespace {

// the live handles: a destroyed one is refused by address, and a call that runs with one keeps it alive until it returns
std::mutex g_control_m;
std::map<gs_host_control *, std::shared_ptr<gs_host_control>> &live_controls() {
    static auto *m = new std::map<gs_host_control *, std::shared_ptr<gs_host_control>>();
    return *m;
}
std::shared_ptr<gs_host_control> live_control(gs_host_control *c) {
    std::lock_guard<std::mutex> l(g_control_m);
    const auto it = live_controls().find(c);
    return it == live_controls().end() ? nullptr : it->second;
}
// (weak: a handle that was destroyed is not mistaken for a later one at the same address)
thread_local std::weak_ptr<gs_host_control> t_attached;

inline int cancelled_rc() { return hfail(GS_E_CANCELLED, "cancelled"); }

// What one file-level call reports: per file the bytes and reads (records, lines) so far.  Without a control attached to the calling
// thread every method is one test of a pointer.  All of it runs on the calling thread.
struct Tracker {
    std::shared_ptr<gs_host_control> hold;
    gs_control::Control *ctl = nullptr;
    std::vector<int64_t> size, done, reads;
    std::vector<double> t_file;
    int files_done = 0;
    double t0 = 0;
    bool on() const { return ctl != nullptr; }
    void begin(const char *const *paths, int n) {
        if (n < 0 || !paths) return;
        hold = t_attached.lock();
        if (!hold || live_control(hold.get()) != hold) return;  // (none attached, or destroyed since)
        ctl = &hold->ctl;
        size.assign((size_t)n, 0);
        done.assign((size_t)n, 0);
        reads.assign((size_t)n, 0);
        t_file.assign((size_t)n, 0);
        for (int i = 0; i < n; i++) {
            struct stat sb;
            if (paths[i] && stat(paths[i], &sb) == 0) size[(size_t)i] = (int64_t)sb.st_size;
        }
        t0 = now_s();
    }
    gs_control::Record record(int f, bool file_done) const {
        gs_control::Record r;
        r.n_files = (int32_t)size.size();
        r.files_done = files_done;
        for (size_t i = 0; i < size.size(); i++) {
            r.total_bytes_done += done[i];
            r.total_bytes_total += size[i];
            r.total_reads += reads[i];
        }
        const double now = now_s();
        r.seconds_total = now - t0;
        if (f >= 0 && (size_t)f < size.size()) {
            r.file = f;
            r.file_done = file_done ? 1 : 0;
            r.file_bytes_done = done[(size_t)f];
            r.file_bytes_total = size[(size_t)f];
            r.file_reads = reads[(size_t)f];
            r.seconds_file = now - t_file[(size_t)f];
        }
        return r;
    }
    bool cancelled() const { return ctl && ctl->cancelled(); }
    // the first record of a file (the reference's start()); true: stop
    bool file_start(int f) {
        if (!ctl) return false;
        t_file[(size_t)f] = now_s();
        return ctl->publish(record(f, false), true);
    }
    // After a chunk or batch whose results are in the state: pos = where the loop stands in the file, in its text (gz: a gzip stream
    // whose stored position nobody knows -- text / 4) or as stored; n = the reads of the file so far.  true: stop
    bool chunk(int f, int64_t pos, bool gz, int64_t n) {
        if (!ctl) return false;
        const int64_t total = size[(size_t)f];
        int64_t at = gz ? std::min(pos / 4, std::max<int64_t>(total - 1, 0)) : pos;
        at = std::min(at, total);
        done[(size_t)f] = std::max(done[(size_t)f], at);
        reads[(size_t)f] = std::max(reads[(size_t)f], n);
        return ctl->publish(record(f, false), false);
    }
    // the last record of a file; true: stop (everything of the file is in the state all the same).  ask = false: the call is being
    // stopped already (another file read side by side saw the flag) -- the record goes out, its answer no longer matters
    bool file_end(int f, int64_t n, bool ask = true) {
        if (!ctl) return false;
        done[(size_t)f] = size[(size_t)f];
        reads[(size_t)f] = n;
        files_done++;
        return ctl->publish(record(f, true), true, ask);
    }
    // the closing record (allDone()): the totals once more, beside the last file's last record
    bool close() {
        if (!ctl) return false;
        return ctl->publish(size.empty() ? record(-1, false) : record((int)size.size() - 1, true), true);
    }
    // the record of a stop: n = exactly the reads of file f that the state covers.  Called when nothing of the file is in flight any
    // more and before its blocks, device text and decoders are released.
    void stopped(int f, int64_t n) {
        if (!ctl) return;
        reads[(size_t)f] = n;
        ctl->publish(record(f, false), true, false);
    }
};
thread_local Tracker *t_tracker = nullptr;
inline Tracker &trk() {
    static Tracker none;  // (never begun: every method returns at its first test)
    return t_tracker ? *t_tracker : none;
}
// the tracker of one file-level call, found by the loops of this thread through trk()
struct TrackerScope {
    Tracker t;
    Tracker *prev;
    TrackerScope(const char *const *paths, int n) : prev(t_tracker) {
        t.begin(paths, n);
        t_tracker = &t;
    }
    ~TrackerScope() { t_tracker = prev; }
};

}  // namespace

extern "C" int gs_host_control_create(gs_host_control **out, gs_host_progress_fn fn, void *user, int32_t every_ms) try {
    if (!out) return hfail(GS_E_INVALID, "NULL argument");
    auto h = std::make_shared<gs_host_control>(fn, user, every_ms);
    std::lock_guard<std::mutex> l(g_control_m);
    live_controls()[h.get()] = h;
    *out = h.get();
    return GS_OK;
} catch (const std::exception &) {
    return hfail(GS_E_NOMEM, "out of host memory");
}

extern "C" int gs_host_control_destroy(gs_host_control *c) {
    std::shared_ptr<gs_host_control> last;  // (dies outside the lock)
    std::lock_guard<std::mutex> l(g_control_m);
    const auto it = live_controls().find(c);
    if (!c || it == live_controls().end()) return hfail(GS_E_INVALID, "not a live control handle");
    last = it->second;
    live_controls().erase(it);
    return GS_OK;
}

extern "C" int gs_host_control_cancel(gs_host_control *c) {
    const auto h = live_control(c);
    if (!h) return hfail(GS_E_INVALID, "not a live control handle");
    h->ctl.cancel();
    return GS_OK;
}

extern "C" int gs_host_control_snapshot(gs_host_control *c, gs_host_progress *out, int32_t *cancelled) {
    const auto h = live_control(c);
    if (!h || !out) return hfail(GS_E_INVALID, h ? "NULL argument" : "not a live control handle");
    gs_control::Record r;
    bool stop = false;
    h->ctl.snapshot(&r, &stop);
    memcpy(out, &r, sizeof r);
    if (cancelled) *cancelled = stop ? 1 : 0;
    return GS_OK;
}

extern "C" int gs_host_control_attach(gs_host_control *c) {
    const auto h = c ? live_control(c) : nullptr;
    if (c && !h) return hfail(GS_E_INVALID, "not a live control handle");
    t_attached = h;
    return GS_OK;
}

namespace {

// ReadEntry.write (AbstractFastqReader.java:570-584) appended to `buf`; qualities are '~' x L unless with_probs and
// present
void append_read(std::vector<uint8_t> &buf, const Batch &b, int64_t i, bool with_probs) {
    const size_t d0 = b.desc_off[i], d1 = b.desc_off[i + 1], s0 = b.seq_off[i], s1 = b.seq_off[i + 1];
    buf.insert(buf.end(), b.desc.begin() + (long)d0, b.desc.begin() + (long)d1);
    buf.push_back('\n');
    buf.insert(buf.end(), b.seq.begin() + (long)s0, b.seq.begin() + (long)s1);
    buf.push_back('\n');
    buf.push_back('+');
    buf.push_back('\n');
    const size_t q0 = b.qual_off[i], q1 = b.qual_off[i + 1];
    if (with_probs && b.has_qual)
        buf.insert(buf.end(), b.qual.begin() + (long)q0, b.qual.begin() + (long)q1);
    else
        buf.insert(buf.end(), s1 - s0, (uint8_t)'~');
    buf.push_back('\n');
}

// bounded producer/consumer hand-off of parsed batches (depth 2: parse i+1 while the GPU works on i)
class BatchQueue {
public:
    void push(std::unique_ptr<Batch> b) {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return q_.size() < 2; });
        q_.push(std::move(b));
        cv_.notify_all();
    }
    std::unique_ptr<Batch> pop() {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return !q_.empty(); });
        auto b = std::move(q_.front());
        q_.pop();
        cv_.notify_all();
        return b;
    }

private:
    std::mutex m_;
    std::condition_variable cv_;
    std::queue<std::unique_ptr<Batch>> q_;
};

}  // namespace


// ---------------------------------------------------------------------------------------------------
// C API
// ---------------------------------------------------------------------------------------------------
struct gs_fastq {
    std::unique_ptr<FastqParser> parser;
    Batch batch;
};

extern "C" int gs_fastq_open(gs_fastq **out, const char *path, int fasta, int k) try {
    if (!out || !path) return hfail(GS_E_INVALID, "NULL argument");
    const bool fa = fasta < 0 ? is_fasta_name(path) : fasta != 0;
    auto r = std::make_unique<gs_fastq>();
    r->parser = std::make_unique<FastqParser>(k, fa);
    if (!r->parser->open(path)) return hfail(GS_E_INVALID, std::string("cannot open ") + path);
    *out = r.release();
    return GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

extern "C" int gs_fastq_next(gs_fastq *r, int64_t max_reads, int64_t max_bytes, gs_read_batch *b) try {
    if (!r || !b) return hfail(GS_E_INVALID, "NULL argument");
    r->parser->parse(r->batch, max_reads, max_bytes);
    b->n_reads = r->batch.n();
    b->seq = r->batch.seq.data();
    b->seq_off = r->batch.seq_off.data();
    b->desc = r->batch.desc.data();
    b->desc_off = r->batch.desc_off.data();
    b->qual = r->batch.qual.data();
    b->qual_off = r->batch.qual_off.data();
    b->first_read_no = r->batch.first_read_no;
    return GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

extern "C" int gs_fastq_totals(const gs_fastq *r, int64_t *reads, int64_t *kmers, int64_t *bps) {
    if (!r) return hfail(GS_E_INVALID, "NULL argument");
    if (reads) *reads = r->parser->reads_;
    if (kmers) *kmers = r->parser->kmers_;
    if (bps) *bps = r->parser->bps_;
    return GS_OK;
}

extern "C" int gs_fastq_close(gs_fastq *r) {
    delete r;
    return GS_OK;
}

extern "C" const char *gs_host_last_error(void) { return g_host_err.c_str(); }

// the ingest path's gzip decoder on a memory range, delivering `block` bytes per decode call (test hook)
extern "C" int gs_host_gunzip(const uint8_t *in, size_t n_in, uint8_t *out, size_t out_cap, size_t *n_out, size_t block) try {
    if ((!in && n_in) || !out || !n_out || block == 0) return hfail(GS_E_INVALID, "bad argument");
    std::unique_ptr<GsInflate> inf(new GsInflate());
    inf->init(in, n_in, true);
    size_t total = 0;
    for (;;) {
        size_t room = out_cap - total;
        if (room > block) room = block;
        size_t p = 0;
        const GsInflate::Status st = inf->decode(out + total, room, total, &p);
        total += p;
        if (st == GsInflate::CORRUPT) return hfail(GS_E_INVALID, "corrupt gzip stream");
        if (st == GsInflate::DONE) break;
        if (total == out_cap) {  // the stream may just have ended: one more call without room tells
            const GsInflate::Status st2 = inf->decode(out + total, 0, total, &p);
            if (st2 == GsInflate::DONE) break;
            return hfail(st2 == GsInflate::CORRUPT ? GS_E_INVALID : GS_E_NOMEM, st2 == GsInflate::CORRUPT ? "corrupt gzip stream" : "output buffer too small");
        }
    }
    *n_out = total;
    return GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}


// the same stream through GsParallelGunzip (test hook): `threads` workers, compressed chunks of `chunk` bytes;
// CRC-32 and ISIZE of every member are checked inside read()
extern "C" int gs_host_gunzip_parallel(const uint8_t *in, size_t n_in, uint8_t *out, size_t out_cap, size_t *n_out, int threads,
                                       size_t chunk, size_t block) try {
    if ((!in && n_in) || !out || !n_out || threads < 1 || block == 0) return hfail(GS_E_INVALID, "bad argument");
    size_t total = 0;
    std::vector<uint8_t> spill(block);
    // BGZF blocks are inflated side by side (GsBgzfReader); ordinary members (behind them, or the whole file) go
    // through the speculative decoder -- the same hand-over as in the file pipeline (TextReader::start_gzip)
    size_t from = 0;
    if (GsBgzfReader::looks_like(in, n_in)) {
        GsBgzfReader bg(in, n_in, threads);
        bool done = false;
        while (!done) {
            uint8_t *dst = total < out_cap ? out + total : spill.data();
            const size_t room = total < out_cap ? std::min(block, out_cap - total) : block;
            size_t p = 0;
            if (!bg.read(dst, room, &p, &done)) return hfail(GS_E_INVALID, "corrupt gzip stream");
            if (dst == spill.data() && p > 0) return hfail(GS_E_NOMEM, "output buffer too small");
            total += p;
        }
        from = bg.rest_offset();
        if (!(from < n_in && n_in - from >= 10 && in[from] == 0x1f && in[from + 1] == 0x8b)) from = n_in;  // trailing garbage
        if (from >= n_in) {
            *n_out = total;
            return GS_OK;
        }
    }
    GsParallelGunzip pg;
    pg.start(in + from, n_in - from, threads, chunk);
    bool done = false;
    while (!done) {
        uint8_t *dst = total < out_cap ? out + total : spill.data();
        const size_t room = total < out_cap ? std::min(block, out_cap - total) : block;
        size_t p = 0;
        if (!pg.read(dst, room, &p, nullptr, &done)) return hfail(GS_E_INVALID, "corrupt gzip stream");
        if (dst == spill.data() && p > 0) return hfail(GS_E_NOMEM, "output buffer too small");
        total += p;
    }
    *n_out = total;
    return GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

namespace {

// parse one source on a producer thread; the consumer gets batches in order; a null batch ends the stream
struct Producer {
    std::thread th;
    BatchQueue q;
    int64_t reads = 0, kmers = 0, bps = 0;
    double seconds = 0;
    std::string error;
    std::atomic<bool> stop{false};  // a stop on request: no further batch is parsed (the consumer drains what is queued)
    // path from byte `offset` on, or the memory range [mem, mem + mem_n) when path is empty
    void start(const std::string &path, int64_t offset, const uint8_t *mem, size_t mem_n, int k, int64_t batch_reads, bool mem_fasta = false) {
        th = std::thread([this, path, offset, mem, mem_n, k, batch_reads, mem_fasta] {
            FastqParser parser(k, path.empty() ? mem_fasta : is_fasta_name(path));
            bool ok_open = true;
            if (path.empty())
                parser.open_mem(mem, mem_n);
            else
                ok_open = parser.open(path, offset);
            if (!ok_open) {
                error = "cannot open " + path;
            } else {
                while (!stop.load()) {
                    auto b = std::make_unique<Batch>();
                    const double t0 = now_s();
                    const bool ok = parser.parse(*b, batch_reads, (int64_t)1 << 30);
                    seconds += now_s() - t0;
                    if (!ok) break;
                    b->src_pos = parser.raw_pos();
                    q.push(std::move(b));
                }
                reads = parser.reads_;  // totalReads += reads (AbstractLoggingFastqStreamer.java:123-125)
                kmers = parser.kmers_;
                bps = parser.bps_;
            }
            q.push(nullptr);
        });
    }
};

}  // namespace

namespace {

// everything one runMatcher call carries from batch to batch
// grow-only array in pinned host memory: per-read results come back from the device into these (a copy into pageable
// memory is staged by the runtime and several times slower); resize() does not keep the contents
template <class T>
struct PinnedVec {
    T *p = nullptr;
    size_t cap = 0, n = 0;
    int resize(size_t m) {
        if (m > cap) {
            gs_pinned_free(p);
            p = nullptr;
            cap = 0;
            void *q = nullptr;
            const size_t want = m + m / 4 + 64;
            const int err = gs_pinned_alloc(&q, want * sizeof(T));
            if (err) return err;
            p = static_cast<T *>(q);
            cap = want;
        }
        n = m;
        return GS_OK;
    }
    T *data() { return p; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
    PinnedVec() = default;
    PinnedVec(const PinnedVec &) = delete;
    PinnedVec &operator=(const PinnedVec &) = delete;
    ~PinnedVec() { gs_pinned_free(p); }
};

// Big page-locked buffers kept from call to call (locking half a gigabyte of pages costs ~0.1 s -- more than a file of four million
// reads takes to filter): get() hands out an idle buffer of at least `bytes` (or allocates), put() takes it back.  Never freed.
struct PinnedPool {
    std::mutex m;
    std::vector<std::pair<void *, size_t>> idle;
    void *get(size_t bytes, size_t *cap) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].second >= bytes) {
                    void *q = idle[i].first;
                    *cap = idle[i].second;
                    idle.erase(idle.begin() + (long)i);
                    return q;
                }
            if (!idle.empty()) {  // too small: give the pages back before asking for more
                gs_pinned_free(idle.back().first);
                idle.pop_back();
            }
        }
        void *q = nullptr;
        const size_t want = bytes + bytes / 8 + 4096;
        if (gs_pinned_alloc(&q, want) != GS_OK) return nullptr;
        *cap = want;
        return q;
    }
    void put(void *q, size_t cap) {
        if (!q) return;
        std::lock_guard<std::mutex> l(m);
        idle.emplace_back(q, cap);
    }
};
inline PinnedPool &pinned_pool() {
    static PinnedPool *p = new PinnedPool();  // (never destroyed: the runtime may be gone by the time statics are torn down)
    return *p;
}
struct PooledBuf {  // one buffer of the pool, returned when it goes out of scope
    void *p = nullptr;
    size_t cap = 0;
    int need(size_t bytes) {
        if (bytes <= cap) return GS_OK;
        pinned_pool().put(p, cap);
        p = pinned_pool().get(bytes, &cap);
        if (!p) {
            cap = 0;
            return hfail(GS_E_NOMEM, "page-locked memory for a text chunk");
        }
        return GS_OK;
    }
    PooledBuf() = default;
    PooledBuf(const PooledBuf &) = delete;
    PooledBuf &operator=(const PooledBuf &) = delete;
    ~PooledBuf() { pinned_pool().put(p, cap); }
};

// ... and the device DEFLATE writers of .gz outputs (slots and output buffer of the size of a chunk's text)
struct DeflaterPool {
    std::mutex m;
    std::vector<std::pair<int, gs_deflater *>> idle;
    gs_deflater *get(int device) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].first == device) {
                    gs_deflater *g = idle[i].second;
                    idle.erase(idle.begin() + (long)i);
                    return g;
                }
        }
        gs_deflater *g = nullptr;
        return gs_deflater_create(&g, device) == GS_OK ? g : nullptr;
    }
    void put(int device, gs_deflater *g) {
        if (!g) return;
        std::lock_guard<std::mutex> l(m);
        idle.emplace_back(device, g);
    }
};
inline DeflaterPool &deflater_pool() {
    static DeflaterPool *p = new DeflaterPool();  // (never destroyed, as the inflaters)
    return *p;
}
// GS_DEVICE_OUTPUT=0: the per-read writers format (and zlib compresses) on host threads, as before round 4
inline bool device_output() {
    if (const char *e = getenv("GS_DEVICE_OUTPUT")) return atoi(e) != 0;
    return true;
}

// GS_DEVICE_KRAKEN=0: the Kraken-style lines are formatted on host threads (and with them the filtered file of the same call, as
// before the lines were made on the device); everything else stays as it is
inline bool device_kraken() {
    if (!device_output()) return false;
    if (const char *e = getenv("GS_DEVICE_KRAKEN")) return atoi(e) != 0;
    return true;
}

// GS_DEVICE_RECORDS=0: the per-read outputs of FASTA and general FASTQ chunks are formatted on host threads (four-line chunks stay
// as GS_DEVICE_OUTPUT / GS_DEVICE_KRAKEN say)
inline bool device_records() {
    if (const char *e = getenv("GS_DEVICE_RECORDS")) return atoi(e) != 0;
    return true;
}

// The device side of one output file of the filter / match goal: the records the file wants have been gathered on the device
// (gs_filter_compact_text / gs_match_compact_text); emit() compresses them there when the file is gzip (gs_deflater_pack: BGZF
// members, what OutFile::pack makes with zlib on host threads) or fetches them as they are, into one of two page-locked buffers,
// and hands that buffer to the file's writer thread by reference.  Called on the chunk's formatting thread, chunk after chunk.
struct DeviceWriter {
    OutFile *out = nullptr;
    int device = 0;
    gs_deflater *defl = nullptr;
    PooledBuf buf[2];
    std::future<void> written[2];
    int flip = 0;
    int64_t bytes_text = 0, bytes_file = 0;
    // text of chunks waits on the device until this much is there (gzip files): 150 chunks of 8 MiB, compressed one by one, were
    // 150 x 0.6 ms of launches and waits (a plain file into a .gz: 4.1 Gbp/s against 12.7 from feeds of 256 MiB)
    static constexpr int64_t kTogether = (int64_t)32 << 20;
    int late_err = GS_OK;  // of a flush the file itself asked for
    std::recursive_mutex mu;
    void begin(OutFile *o, int dev) {
        out = o;
        device = dev;
        if (out) out->before_host_write = [this] {
            const int e = flush_pending();
            if (e && !late_err) late_err = e;
        };
    }
    // n_out bytes of buf[flip] to the file's writer thread, by reference
    void hand_over(int64_t n_out) {
        auto pr = std::make_shared<std::promise<void>>();
        written[flip] = pr->get_future();
        out->write_ref(static_cast<const uint8_t *>(buf[flip].p), (size_t)n_out, [pr] { pr->set_value(); });
        bytes_file += n_out;
        flip ^= 1;
    }
    int flush_pending() {
        std::lock_guard<std::recursive_mutex> l(mu);
        const int64_t n = defl ? gs_deflater_pending(defl) : 0;
        if (n <= 0) return GS_OK;
        if (written[flip].valid()) written[flip].get();  // (the buffer before last is on disk)
        const int64_t cap = gs_deflate_bound(n);
        int err = buf[flip].need((size_t)cap);
        if (err) return err;
        int64_t n_out = 0;
        if (gs_deflater_flush(defl, static_cast<uint8_t *>(buf[flip].p), cap, &n_out) != GS_OK)
            return hfail(GS_E_HIP, std::string("device DEFLATE writer: ") + gs_deflate_last_error());
        hand_over(n_out);
        return GS_OK;
    }
    // (set: the caller's chunk parity -- d_text stays valid until the chunk after next is gathered; nothing here depends on it)
    int emit(int set, const uint8_t *d_text, int64_t n_bytes) {
        (void)set;
        if (!out || !out->active() || n_bytes <= 0) return GS_OK;
        std::lock_guard<std::recursive_mutex> l(mu);
        if (late_err) return late_err;
        bytes_text += n_bytes;
        if (out->gzip()) {
            if (!defl && !(defl = deflater_pool().get(device))) return hfail(GS_E_NOMEM, "no device DEFLATE writer");
            if (n_bytes >= kTogether && gs_deflater_pending(defl) == 0) {  // enough for a call of its own: from where it lies
                if (written[flip].valid()) written[flip].get();
                const int64_t cap = gs_deflate_bound(n_bytes);
                int err = buf[flip].need((size_t)cap);
                if (err) return err;
                int64_t n_out = 0;
                if (gs_deflater_pack(defl, d_text, n_bytes, static_cast<uint8_t *>(buf[flip].p), cap, &n_out) != GS_OK)
                    return hfail(GS_E_HIP, std::string("device DEFLATE writer: ") + gs_deflate_last_error());
                hand_over(n_out);
                return GS_OK;
            }
            if (gs_deflater_append(defl, d_text, n_bytes) != GS_OK) return hfail(GS_E_HIP, std::string("device DEFLATE writer: ") + gs_deflate_last_error());
            return gs_deflater_pending(defl) >= kTogether ? flush_pending() : GS_OK;
        }
        if (written[flip].valid()) written[flip].get();
        int err = buf[flip].need((size_t)n_bytes);
        if (err) return err;
        if (gs_device_fetch(device, d_text, static_cast<uint8_t *>(buf[flip].p), n_bytes) != GS_OK) return hfail(GS_E_HIP, gs_inflate_last_error());
        hand_over(n_bytes);
        return GS_OK;
    }
    // what still waits is compressed, every buffer handed to the writer thread has been written; the deflater goes back to its pool
    int finish() {
        std::lock_guard<std::recursive_mutex> l(mu);
        int err = late_err;
        if (out && out->active()) {
            const int e = flush_pending();
            if (!err) err = e;
        }
        if (out) out->before_host_write = nullptr;
        for (auto &w : written)
            if (w.valid()) w.get();
        if (defl) {
            if (gs_deflater_pending(defl) > 0) {  // (an error on the way: nothing of this file may wait in a pooled object)
                int64_t dummy = 0;
                PooledBuf tmp;
                if (tmp.need((size_t)gs_deflate_bound(gs_deflater_pending(defl))) == GS_OK)
                    gs_deflater_flush(defl, static_cast<uint8_t *>(tmp.p), gs_deflate_bound(gs_deflater_pending(defl)), &dummy);
            }
            deflater_pool().put(device, defl);
        }
        defl = nullptr;
        return err;
    }
    ~DeviceWriter() { finish(); }
};

struct MatchCtx {
    gs_run *run = nullptr;
    gs_db_info info{};
    const gs_host_match_opts *opts = nullptr;
    OutFile filtered, kraken;
    // per-read results of a batch; two sets, so that the writers can work on one chunk while the device fills the
    // other (TextJob)
    struct Results {
        PinnedVec<int32_t> cls, seg_code, seg_start;
        PinnedVec<uint8_t> flags;
        PinnedVec<uint64_t> seg_off;
        PinnedVec<uint32_t> nl;
    } res[2];
    FormatPool pool{format_threads()};  // the per-read writers format a batch on these threads
    std::vector<uint32_t> taxid_len;    // strlen of opts->taxids[vi] (Kraken-style lines)
    size_t taxid_max = 1;
    int64_t global_read_no = 0, filtered_reads = 0;  // read numbers run over all files of the call (file order)
    int64_t reads = 0, kmers = 0, bps = 0;
    double t_gpu = 0, t_parse = 0;
    DeviceWriter filtered_dev;  // the filtered file fed from the device (TextJob::emit_device)
    DeviceWriter kraken_dev;    // the Kraken-style lines made on the device (gs_match_kraken_text), a deflater of its own
    bool taxids_on_device = false;  // gs_match_set_taxids has been called for this run
    // progress records of the general parser (parsed_source): the file it works for, and the number of that file's first read
    int prog_file = 0;
    int64_t prog_base = 0;
    // CountsPerTaxid.maxContigDescriptor for a host that never sees the reads (opts->max_contig_desc): after every chunk the device
    // names the read that holds each tax id's longest contig (gs_match_max_contig_reads); a holder that lies in the chunk just
    // submitted gets its name fetched while the chunk's text is at hand.  A maximum only moves to a later read by beating it, so
    // the name kept at the end is the one gs_match_finish's read number stands for.
    std::vector<int64_t> max_holder, max_now;
    bool track_desc() const { return opts && opts->max_contig_desc != nullptr && opts->max_contig_desc_stride >= 2; }
    // fetch(records in the chunk, n, out, stride) -> the records' descriptor lines, NUL-terminated; null: the text is not at hand
    int update_max_contig(int64_t first_no, int64_t n_reads, const std::function<int(const int64_t *, int32_t, uint8_t *, int32_t)> &fetch) {
        if (!track_desc() || n_reads <= 0) return GS_OK;
        const size_t nv = (size_t)info.n_values;
        if (max_holder.size() != nv) max_holder.assign(nv, -1);
        max_now.resize(nv);
        int err = gs_match_max_contig_reads(run, max_now.data());
        if (err) return err;
        std::vector<int64_t> recs;
        std::vector<size_t> vis;
        for (size_t v = 0; v < nv; v++) {
            const int64_t r = max_now[v];
            if (r != max_holder[v] && r >= first_no && r < first_no + n_reads) {
                recs.push_back(r - first_no);
                vis.push_back(v);
            }
            max_holder[v] = r;
        }
        if (recs.empty()) return GS_OK;
        const int32_t stride = opts->max_contig_desc_stride;
        std::vector<uint8_t> lines(recs.size() * (size_t)stride + 1, 0);
        if (fetch && (err = fetch(recs.data(), (int32_t)recs.size(), lines.data(), stride))) return err;
        for (size_t i = 0; i < recs.size(); i++) {
            const uint8_t *l = lines.data() + i * (size_t)stride;
            uint8_t *o = opts->max_contig_desc + vis[i] * (size_t)stride;
            int32_t j = 1;  // (behind the line's first character, up to the first blank: FastqKMerMatcher.java:404-407)
            for (; l[0] && j < stride && l[j] && l[j] != ' '; j++) o[j - 1] = l[j];
            o[j - 1] = 0;
        }
        return GS_OK;
    }
};

// MatcherReadEntry.writeMatchDetails (:723-756) for read i of the current batch / chunk (c.cls, c.seg_*): descriptor
// up to the first blank without its '@', class taxid, length, runs "taxid:n"
inline uint8_t *put_uint(uint8_t *o, uint64_t v) {
    char tmp[20];
    int n = 0;
    do {
        tmp[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *o++ = (uint8_t)tmp[--n];
    return o;
}

void kraken_line(const MatchCtx &c, const MatchCtx::Results &rs, std::vector<uint8_t> &out, const uint8_t *desc, size_t dlen,
                 int64_t L, int64_t i) {
    const gs_host_match_opts *opts = c.opts;
    const uint64_t s0 = rs.seg_off[(size_t)i], s1 = rs.seg_off[(size_t)i + 1];
    const int32_t cl = rs.cls[(size_t)i];
    if (s1 == s0 || !(opts->write_all || cl >= 0)) return;
    const int64_t maxp = L - c.info.k + 1;
    // written in place: make room for the longest this line can get, cut back to what it took
    const size_t at = out.size();
    const size_t room = 2 + dlen + 1 + c.taxid_max + 1 + 20 + 1 + (size_t)(s1 - s0) * (c.taxid_max + 23) + 1;
    if (out.capacity() < at + room) out.reserve(std::max(2 * out.capacity(), at + room + ((size_t)1 << 16)));
    out.resize(at + room);
    uint8_t *o = out.data() + at;
    *o++ = cl >= 0 ? 'C' : 'U';
    *o++ = '\t';
    if (dlen > 1) {
        const void *sp = memchr(desc + 1, ' ', dlen - 1);
        const size_t n = sp ? (size_t)((const uint8_t *)sp - desc) - 1 : dlen - 1;
        memcpy(o, desc + 1, n);
        o += n;
    }
    *o++ = '\t';
    if (cl >= 0) {
        memcpy(o, opts->taxids[cl], c.taxid_len[(size_t)cl]);
        o += c.taxid_len[(size_t)cl];
    } else
        *o++ = '0';
    *o++ = '\t';
    o = put_uint(o, (uint64_t)L);
    *o++ = '\t';
    for (uint64_t sg = s0; sg < s1; sg++) {
        if (sg > s0) *o++ = ' ';
        const int32_t code = rs.seg_code[(size_t)sg];
        if (code == -2)
            *o++ = 'A';
        else if (code < 0)
            *o++ = '0';
        else {
            memcpy(o, opts->taxids[code], c.taxid_len[(size_t)code]);
            o += c.taxid_len[(size_t)code];
        }
        *o++ = ':';
        const int64_t cnt = (sg + 1 < s1 ? rs.seg_start[(size_t)sg + 1] : maxp) - rs.seg_start[(size_t)sg];
        if (cnt < 0) *o++ = '-';  // (cannot happen for segments the device produced; printed like the reference's int)
        o = put_uint(o, (uint64_t)(cnt < 0 ? -cnt : cnt));
    }
    *o++ = '\n';
    out.resize((size_t)(o - out.data()));
}

// per-thread output of one batch: Kraken lines and filtered records of a contiguous range of reads
struct FormatPart {
    std::vector<uint8_t> kraken, filtered;
    bool kraken_packed = false, filtered_packed = false;  // already a gzip member (OutFile::pack)
    int64_t n_filtered = 0;
    // a part that is big enough is compressed by the thread that made it
    void pack(OutFile &kr, OutFile &flt) {
        const size_t worth_it = (size_t)64 << 10;
        kraken_packed = kr.gzip() && kraken.size() >= worth_it && kr.pack(kraken);
        filtered_packed = flt.gzip() && filtered.size() >= worth_it && flt.pack(filtered);
    }
};

// hands the parts to the writers in read order
void write_parts(MatchCtx &c, std::vector<FormatPart> &parts) {
    for (FormatPart &p : parts) {
        c.filtered_reads += p.n_filtered;
        c.filtered.write(std::move(p.filtered), p.filtered_packed);
        c.kraken.write(std::move(p.kraken), p.kraken_packed);
    }
}

// one parsed batch through the GPU and the per-read writers
int consume_batch(MatchCtx &c, Batch &b, int64_t &read_no) {
    const int64_t n = b.n();
    MatchCtx::Results &rs = c.res[0];
    int err = rs.cls.resize((size_t)n);
    if (!err) err = rs.flags.resize((size_t)n);
    if (err) return err;
    if (b.seq.empty()) b.seq.push_back(0);
    const double t0 = now_s();
    err = gs_match_submit(c.run, b.seq.data(), b.seq_off.data(), n, read_no, GS_MEM_HOST, rs.cls.data(), rs.flags.data());
    if (!err && c.kraken.active()) {
        err = rs.seg_off.resize((size_t)n + 1);
        if (!err) err = gs_match_segments(c.run, b.seq.data(), b.seq_off.data(), n, GS_MEM_HOST, rs.seg_off.data());
        if (!err) err = rs.seg_code.resize((size_t)rs.seg_off[(size_t)n]);
        if (!err) err = rs.seg_start.resize((size_t)rs.seg_off[(size_t)n]);
        if (!err) err = gs_match_segments_fetch(c.run, rs.seg_code.data(), rs.seg_start.data());
    }
    c.t_gpu += now_s() - t0;
    if (err) return err;
    err = c.update_max_contig(read_no, n, [&b](const int64_t *recs, int32_t m, uint8_t *out, int32_t stride) {
        for (int32_t i = 0; i < m; i++) {
            const size_t d0 = b.desc_off[(size_t)recs[i]], d1 = b.desc_off[(size_t)recs[i] + 1];
            const size_t len = std::min<size_t>(d1 - d0, (size_t)stride - 1);
            memcpy(out + (size_t)i * (size_t)stride, b.desc.data() + d0, len);
            out[(size_t)i * (size_t)stride + len] = 0;
        }
        return (int)GS_OK;
    });
    if (err) return err;
    read_no += n;
    if (!c.filtered.active() && !c.kraken.active()) return GS_OK;
    std::vector<FormatPart> parts((size_t)c.pool.threads());
    c.pool.run(n, [&](int t, int64_t lo, int64_t hi) {
        FormatPart &p = parts[(size_t)t];
        p.filtered = c.filtered.take();
        p.kraken = c.kraken.take();
        for (int64_t i = lo; i < hi; i++) {
            if (c.filtered.active() && (rs.flags[(size_t)i] & GS_F_RETURNED)) {  // afterMatch (:304-307)
                append_read(p.filtered, b, i, c.opts->with_probs != 0);
                p.n_filtered++;
            }
            if (c.kraken.active()) {
                const size_t d0 = b.desc_off[(size_t)i], d1 = b.desc_off[(size_t)i + 1];
                const int64_t L = (int64_t)(b.seq_off[(size_t)i + 1] - b.seq_off[(size_t)i]);
                kraken_line(c, rs, p.kraken, b.desc.data() + d0, d1 - d0, L, i);
            }
        }
        p.pack(c.kraken, c.filtered);
    });
    write_parts(c, parts);
    return GS_OK;
}

// the general path: the reference's record parser on a producer thread (file from `offset`, or a memory range)
int parsed_source(MatchCtx &c, const std::string &path, int64_t offset, const uint8_t *mem, size_t mem_n, int64_t &read_no,
                  bool mem_fasta = false) {
    Producer prod;
    prod.start(path, offset, mem, mem_n, c.info.k, c.opts->batch_reads > 0 ? c.opts->batch_reads : (int64_t)1 << 20, mem_fasta);
    int err = GS_OK;
    Tracker &tk = trk();
    int64_t seen[3] = {0, 0, 0};  // reads, k-mers, bases of the batches that went through (what counts after a stop)
    bool stopped = false;
    for (;;) {
        std::unique_ptr<Batch> b = prod.q.pop();
        if (!b) break;
        if (err) continue;  // keep draining so the producer can finish
        err = consume_batch(c, *b, read_no);
        if (!err && tk.on()) {
            for (int64_t i = 0; i < b->n(); i++) {
                const int64_t L = (int64_t)(b->seq_off[(size_t)i + 1] - b->seq_off[(size_t)i]);
                seen[1] += L >= c.info.k ? L - c.info.k + 1 : 0;
                seen[2] += L;
            }
            seen[0] += b->n();
            if (tk.chunk(c.prog_file, path.empty() ? 0 : b->src_pos, false, read_no - c.prog_base)) {
                prod.stop.store(true);  // (what it has parsed beyond this batch is dropped, above)
                stopped = true;
                err = GS_E_CANCELLED;
            }
        }
    }
    prod.th.join();
    if (stopped) {  // every batch was waited for (consume_batch); the run holds exactly the reads in front of read_no
        c.reads += seen[0];
        c.kmers += seen[1];
        c.bps += seen[2];
        c.t_parse += prod.seconds;
        gs_match_sync(c.run);
        tk.stopped(c.prog_file, read_no - c.prog_base);
        return cancelled_rc();
    }
    if (!err && !prod.error.empty()) err = hfail(GS_E_INVALID, prod.error);
    c.reads += prod.reads;
    c.kmers += prod.kmers;
    c.bps += prod.bps;
    c.t_parse += prod.seconds;
    return err;
}

std::atomic<int64_t> g_ml_chunks{0};  // chunks matched through the general FASTQ device path (gs_host_stat(0))
std::atomic<int64_t> g_filter_general_chunks{0};  // FASTA / general FASTQ chunks filtered on the device (gs_host_stat(1))
std::atomic<int64_t> g_kraken_device_chunks{0};  // chunks whose Kraken-style lines were written on the device (gs_host_stat(2))
std::atomic<int64_t> g_krakencount_chunks{0};  // chunks of Kraken-style lines counted on the device (gs_host_stat(5))
std::atomic<int64_t> g_record_device_chunks{0};  // FASTA / general FASTQ chunks whose per-read output was written on the device (gs_host_stat(3))

struct TextChunk {
    int64_t file_off;  // of the chunk's first byte
    int64_t reads_before;  // reads of this file in earlier chunks
    int64_t ticket;
};

// ReadEntry.write of record i of a raw chunk (newline offsets nl[]): descriptor, read, "+", then '~' x length or
// (with_probs) the record's quality line -- in a chunk the device accepted that is ONE line at least as long as the read
// (appended to `buf`; the caller writes one buffer per chunk)
void append_text_record(std::vector<uint8_t> &buf, const uint8_t *text, const uint32_t *nl, int64_t i, bool with_probs) {
    const size_t d0 = i == 0 ? 0 : (size_t)nl[4 * i - 1] + 1, d1 = nl[4 * i], s0 = d1 + 1, s1 = nl[4 * i + 1];
    const size_t at = buf.size(), dl = d1 - d0, sl = s1 - s0;
    if (with_probs) {
        const size_t q0 = (size_t)nl[4 * i + 2] + 1, ql = (size_t)nl[4 * i + 3] - q0;
        buf.resize(at + dl + sl + ql + 5);
        uint8_t *o = buf.data() + at;
        memcpy(o, text + d0, dl + 1 + sl + 1);  // descriptor and read lines as they stand, newlines included
        o += dl + sl + 2;
        *o++ = '+';
        *o++ = '\n';
        memcpy(o, text + q0, ql + 1);
        return;
    }
    buf.resize(at + dl + 2 * sl + 5);
    uint8_t *o = buf.data() + at;
    memcpy(o, text + d0, dl);
    o += dl;
    *o++ = '\n';
    memcpy(o, text + s0, sl);
    o += sl;
    *o++ = '\n';
    *o++ = '+';
    *o++ = '\n';
    memset(o, '~', sl);
    o += sl;
    *o = '\n';
}

// One FASTQ file (plain or gzip) going to the device as raw text blocks.  Falls back to
// parsed_source() from the first chunk the device refuses (gs_match_text_status), so any file the general path accepts
// gives the same result.  step() handles one block; several jobs can be stepped in turn (files read side by side),
// each with its own status bank on the device and its own range of read numbers.
// One record of a FASTA or general FASTQ chunk as four-line FASTQ (ReadEntry.write, AbstractFastqReader.java:570-584): lines h
// (descriptor) to next - 1 of the chunk, newline offsets nl, line classes cls (1 descriptor, 2 sequence, 0 '+' / quality), read
// length L.  Descriptor (FASTA: '>' replaced by '@', :380), the read in ONE line, "+", then the quality characters of the record
// (general FASTQ with withProbs: every quality line that was consumed, joined) or '~' x length.
void append_general_record(std::vector<uint8_t> &o, const uint8_t *text, const uint32_t *nl, const uint8_t *cls, int64_t h, int64_t next,
                           int64_t L, bool is_fasta, bool probs) {
    auto line_start = [nl](int64_t i) { return i ? (size_t)nl[i - 1] + 1 : (size_t)0; };
    const size_t d0 = line_start(h), dlen = (size_t)nl[h] - d0, at = o.size();
    o.insert(o.end(), text + d0, text + d0 + dlen);
    if (is_fasta && dlen > 0) o[at] = '@';
    o.push_back('\n');
    int64_t i = h + 1;
    for (; i < next && cls[(size_t)i] == 2; i++) o.insert(o.end(), text + line_start(i), text + nl[i]);
    o.push_back('\n');
    o.push_back('+');
    o.push_back('\n');
    if (probs) {
        for (i++; i < next; i++) o.insert(o.end(), text + line_start(i), text + nl[i]);  // (behind the '+' line)
    } else
        o.insert(o.end(), (size_t)L, (uint8_t)'~');
    o.push_back('\n');
}

// `job` on a thread of its own, its result in `fut`; on this thread where no thread is to be had
template <class T, class F>
void run_behind(std::future<T> &fut, F job) {
    try {
        fut = std::async(std::launch::async, job);
    } catch (const std::system_error &) {
        fut = std::async(std::launch::deferred, job);
        fut.wait();
    }
}

// block size and reader / inflating threads of the text pipelines (GS_HOST_BLOCK_BYTES, GS_HOST_READERS); readers > 0 on entry: the
// caller's own default.  Measured on the MI355X box (tools/file_rate_sweep.sh, 5 GB file in the page cache): 8 readers x 8 MiB blocks
// 24.8 GB/s of file, 4 x 32 MiB 10.6 GB/s, 8 x 128 MiB 9.1 GB/s -- blocks that stay in the CPU caches between pread and the newline
// count win
void reader_shape(bool gzip, size_t *block, int *readers) {
    *block = (size_t)8 << 20;
    if (const char *e = getenv("GS_HOST_BLOCK_BYTES")) {
        const long long v = atoll(e);
        if (v >= 64 && v <= ((long long)1 << 29)) *block = (size_t)v;
    }
    if (*readers <= 0) *readers = (int)std::min<unsigned>(gzip ? 16 : 8, std::max<unsigned>(2, std::thread::hardware_concurrency() / 2));
    if (const char *e = getenv("GS_HOST_READERS")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 32) *readers = v;
    }
}

// GS_OK, or what went wrong with the block the reader has just delivered
int block_error(TextReader &tr, const TextSlot &sl, const std::string &path) {
    if (!sl.io_error && tr.verify_gzip(sl)) return GS_OK;
    return hfail(tr.gz ? GS_E_INVALID : GS_E_IO, (tr.gz ? "corrupt gzip stream in " : "read error on ") + path);
}

// the next chunk of a file out of reader block `sl` (ChunkCutter::next)
ChunkCutter::Cut cut_block(ChunkCutter &cut, const TextReader &tr, const TextSlot &sl) {
    return cut.next(sl.buf + tr.headroom, (int64_t)sl.n, sl.newlines, sl.last4, sl.eof, tr.headroom);
}

// device inflaters are kept for the life of the process, per device: their buffers (two text buffers, two staging buffers, page-locked
// mirrors) take longer to allocate and free than a file takes to inflate
struct InflaterPool {
    std::mutex m;
    std::vector<std::pair<int, gs_inflater *>> idle;
    gs_inflater *get(int device) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].first == device) {
                    gs_inflater *g = idle[i].second;
                    idle.erase(idle.begin() + (long)i);
                    return g;
                }
        }
        gs_inflater *g = nullptr;
        return gs_inflater_create(&g, device) == GS_OK ? g : nullptr;
    }
    void put(int device, gs_inflater *g) {
        if (gs_inflater_reset(g) != GS_OK) {
            gs_inflater_destroy(g);
            return;
        }
        std::lock_guard<std::mutex> l(m);
        idle.emplace_back(device, g);
    }
};
// ... and the decoders of single-member streams, whose device buffers are gigabytes (one idle object per device is kept)
struct GunzipperPool {
    std::mutex m;
    std::vector<std::pair<int, gs_gunzipper *>> idle;
    int open(gs_gunzipper **out, int device, const uint8_t *gz, int64_t n) {
        gs_gunzipper *g = nullptr;
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < idle.size(); i++)
                if (idle[i].first == device) {
                    g = idle[i].second;
                    idle.erase(idle.begin() + (long)i);
                    break;
                }
        }
        if (g) {
            const int rc = gs_gunzipper_reopen(g, gz, n);
            if (rc == GS_OK) {
                *out = g;
                return GS_OK;
            }
            gs_gunzipper_close(g);
            *out = nullptr;
            return rc;
        }
        return gs_gunzipper_open(out, device, gz, n);
    }
    void put(int device, gs_gunzipper *g) {
        if (!g) return;
        gs_gunzipper_park(g);  // (the file is about to be unmapped: no upload thread may read it any more)
        {
            std::lock_guard<std::mutex> l(m);
            bool have = false;
            for (auto &x : idle) have = have || x.first == device;
            if (!have) {
                idle.emplace_back(device, g);
                return;
            }
        }
        gs_gunzipper_close(g);
    }
};
// compressed bytes of a stream's first batch when writers wait for its text (GS_HOST_GUNZIP_FIRST; 0: a full batch)
inline int64_t gunzip_first_span() {
    if (const char *e = getenv("GS_HOST_GUNZIP_FIRST")) return std::max<int64_t>(0, atoll(e));
    return (int64_t)64 << 20;
}

// ... and when nobody waits for it but the match kernel (GS_HOST_GUNZIP_FIRST_MATCH; 0: a full batch): the first batch is the only one
// that waits for its compressed bytes to cross PCIe
inline int64_t gunzip_first_span_match() {
    if (const char *e = getenv("GS_HOST_GUNZIP_FIRST_MATCH")) return std::max<int64_t>(0, atoll(e));
    return 0;
}

inline GunzipperPool &gunzipper_pool() {
    static GunzipperPool *p = new GunzipperPool();  // (never destroyed, as the inflaters)
    return *p;
}

inline InflaterPool &inflater_pool() {
    static InflaterPool *p = new InflaterPool();  // (never destroyed: the runtime may be gone by the time statics are torn down)
    return *p;
}

// every byte of the mapped file belongs to a BGZF member: list them (payload, ISIZE, CRC-32); false: not (only) BGZF
inline bool bgzf_member_list(const uint8_t *map, size_t map_len, std::vector<gs_inflate_member> &members) {
    members.clear();
    size_t o = 0;
    while (o < map_len) {
        size_t len = 0;
        uint32_t isize = 0;
        if (!GsBgzfReader::block_at(map, map_len, o, &len, &isize)) return false;
        const uint8_t *p = map + o;
        if (p[3] != 4) return false;  // (name / comment / header CRC: not what bgzip writes -- the general decoder knows them)
        const size_t hdr = 12 + ((size_t)p[10] | ((size_t)p[11] << 8));
        const uint8_t *t = p + len - 8;
        gs_inflate_member m{};
        m.payload_offset = (int64_t)(o + hdr);
        m.payload_len = (uint32_t)(len - hdr - 8);
        m.isize = isize;
        m.crc32 = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        if (isize > 0) members.push_back(m);
        o += len;
    }
    return !members.empty();
}

// text per feed of the device inflater (GS_HOST_BGZF_TEXT): a feed is ~8000 members at 512 MiB, two rounds over the device's wave slots
inline int64_t bgzf_text_target() {
    int64_t t = (int64_t)512 << 20;
    if (const char *e = getenv("GS_HOST_BGZF_TEXT")) {
        const long long v = atoll(e);
        if (v >= 65536 && v <= ((long long)1 << 29)) t = v;
    }
    return t;
}

// What a device-inflated source hands out per call: n_lines whole four-line lines in n_bytes of text that lies on the device.
struct DevText {
    const uint8_t *text = nullptr;
    int64_t n_bytes = 0, n_lines = 0;
    bool last = false;   // the file is through: what lies behind the text is the leftover
    bool stuck = false;  // no whole record and no end in sight: the general parser from here
};

// Block-gzip (BGZF) input: the members are listed from their headers, runs of them go to the device COMPRESSED and are inflated
// there (gs_inflater_feed, one wave per member); the inflater keeps what lies behind a feed's last whole record for the next one.
struct BgzfFeeds {
    gs_inflater *inf = nullptr;
    int device = 0;
    const uint8_t *map = nullptr;
    std::vector<gs_inflate_member> members;
    size_t next_member = 0;
    int64_t n_feeds = 0, tail = 0;
    // the run of members from `from` whose text stays within the target (one member at least)
    size_t run_end(size_t from, int64_t text_target) const {
        int64_t sum = 0;
        size_t e = from;
        while (e < members.size() && (e == from || sum + members[e].isize <= text_target)) sum += members[e++].isize;
        return e;
    }
    // the next run, and a look ahead at the one behind it (its compressed bytes are uploaded meanwhile)
    int next(int64_t text_target, const std::string &path, DevText *t) {
        const size_t a = next_member, b = run_end(a, text_target), b2 = run_end(b, text_target);
        int64_t next_lo = 0, next_hi = 0;
        if (b2 > b) {
            next_lo = members[b].payload_offset;
            next_hi = members[b2 - 1].payload_offset + (int64_t)members[b2 - 1].payload_len;
        }
        *t = DevText{};
        t->last = b == members.size();
        n_feeds++;
        next_member = b;
        if (gs_inflater_feed(inf, map, members.data() + a, (int64_t)(b - a), next_lo, next_hi, t->last ? 1 : 0, &t->text, &t->n_bytes, &t->n_lines, &tail) != GS_OK)
            return hfail(GS_E_INVALID, std::string("corrupt gzip stream in ") + path + ": " + gs_inflate_last_error());
        t->stuck = t->n_lines == 0 && tail > ((int64_t)256 << 20) && !t->last;  // no record boundary in a quarter of a gigabyte
        return GS_OK;
    }
    int fetch_text(uint8_t *dst, int64_t n_bytes) { return gs_inflater_fetch(inf, dst, n_bytes) == GS_OK ? (int)GS_OK : hfail(GS_E_HIP, gs_inflate_last_error()); }
    // what is left behind the last whole record
    int fetch_tail(std::vector<uint8_t> &carry) {
        int64_t n = 0;
        carry.resize((size_t)tail);
        return tail == 0 || gs_inflater_tail(inf, carry.data(), tail, &n) == GS_OK ? (int)GS_OK : hfail(GS_E_HIP, gs_inflate_last_error());
    }
    void close() {
        if (inf) inflater_pool().put(device, inf);
        inf = nullptr;
    }
};

// A gzip stream inflated on the device as a whole (gs_gunzip_plan_device: block starts found speculatively, segments decoded side by
// side, windows resolved in a second pass; members behind one another each with their own CRC-32 / ISIZE): its text lies in HBM,
// batch after batch (gs_gunzipper_next), and is handed on in slices of whole four-line records.
struct GunzipSlices {
    gs_gunzipper *gzr = nullptr;
    int device = 0;
    const uint8_t *gz_text = nullptr;  // the current batch
    int64_t gz_n = 0, gz_off = 0;
    int gz_last = 0;  // 1: the current batch is the file's last
    // The next slice: whole records up to the feed size, from this batch or with the next one behind what is left of this.  A new
    // batch replaces the text of the last: before_replace() (may be null) waits for whoever still reads that.  *refused: a batch the
    // device path does not take -- the host decoders from the start of what was left.
    int next(int64_t text_target, const std::string &path, const std::function<int()> &before_replace, DevText *t, bool *refused) {
        *t = DevText{};
        *refused = false;
        for (;;) {
            const int64_t rest = gz_n - gz_off, look = std::min(rest, text_target);
            t->n_lines = t->n_bytes = 0;
            if (look > 0 && gs_text_cut_device(device, gz_text + gz_off, look, &t->n_lines, &t->n_bytes) != GS_OK) return hfail(GS_E_HIP, gs_inflate_last_error());
            if (t->n_lines > 0 || gz_last || look < rest) break;  // (look < rest: a full slice without a record -- `stuck`, below)
            if (before_replace) {
                const int err = before_replace();
                if (err) return err;
            }
            const int grc = gs_gunzipper_next(gzr, rest, &gz_text, &gz_n, &gz_last);
            gz_off = 0;
            if (grc == GS_E_UNSUPPORTED || grc == GS_E_NOMEM) {  // (the tail that was kept belongs to the host decoders as well)
                gz_n = 0;
                *refused = true;
                return GS_OK;
            }
            if (grc != GS_OK) return hfail(GS_E_INVALID, std::string("corrupt gzip stream in ") + path + ": " + gs_inflate_last_error());
        }
        const int64_t rest = gz_n - gz_off;
        t->last = gz_last != 0 && std::min(rest, text_target) == rest;
        t->stuck = t->n_lines == 0 && !t->last;
        t->text = gz_text + gz_off;
        gz_off += t->n_bytes;
        return GS_OK;
    }
    int fetch_text(const DevText &t, uint8_t *dst) { return gs_device_fetch(device, t.text, dst, t.n_bytes) == GS_OK ? (int)GS_OK : hfail(GS_E_HIP, gs_inflate_last_error()); }
    // what is left behind the last slice
    int fetch_leftover(std::vector<uint8_t> &carry) {
        const int64_t n = gz_n - gz_off;
        carry.resize((size_t)n);
        return n == 0 || gs_device_fetch(device, gz_text + gz_off, carry.data(), n) == GS_OK ? (int)GS_OK : hfail(GS_E_HIP, gs_inflate_last_error());
    }
    // Back to the pool, which parks the upload thread: it copies from the mapped file (a stream of up to 16 GiB is uploaded whole
    // while the batches run), so this comes BEFORE the file is unmapped -- and after everybody is through with the device text.
    void close() {
        if (gzr) gunzipper_pool().put(device, gzr);
        gzr = nullptr;
        gz_text = nullptr;
        gz_n = gz_off = 0;
    }
};

// Whether and how a gzip file of four-line FASTQ is inflated on the device: block-gzip by its members, any other stream as a whole,
// or not at all -- GS_DEVICE_INFLATE=0, GS_DEVICE_GUNZIP=0 (whole streams), no pooled object to be had, or a stream the device path
// does not take (a damaged one too): the host decoders then inflate it as before, and report it.  close() before the file is unmapped.
struct DeviceInflate {
    BgzfFeeds feeds;
    GunzipSlices slices;
    bool bgzf() const { return feeds.inf != nullptr; }
    bool whole() const { return slices.gzr != nullptr; }
    // first_span: compressed bytes of a whole stream's first batch, the only one that waits for its bytes to cross PCIe
    void open(const uint8_t *map, size_t map_len, int device, int64_t first_span) {
        bool want = true, want_whole = true;
        if (const char *e = getenv("GS_DEVICE_INFLATE")) want = atoi(e) != 0;
        if (const char *e = getenv("GS_DEVICE_GUNZIP")) want_whole = atoi(e) != 0;
        if (!want || map_len < 18) return;
        if (map_len >= 28 && bgzf_member_list(map, map_len, feeds.members)) {
            feeds.inf = inflater_pool().get(device);
            feeds.device = device;
            feeds.map = map;
            return;
        }
        feeds.members.clear();
        if (!want_whole) return;
        static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
        const double tg = now_s();
        slices.device = device;
        int grc = gunzipper_pool().open(&slices.gzr, device, map, (int64_t)map_len);
        if (grc == GS_OK) grc = gs_gunzipper_first_span(slices.gzr, first_span);
        if (grc == GS_OK) grc = gs_gunzipper_next(slices.gzr, 0, &slices.gz_text, &slices.gz_n, &slices.gz_last);  // (the first batch now: a stream this path does not take shows here)
        if (trace)
            fprintf(stderr, "gunzip on the device: rc %d, first batch %lld bytes of text, %.2f ms%s%s\n", grc, (long long)slices.gz_n, (now_s() - tg) * 1e3, grc ? ": " : "",
                    grc ? gs_inflate_last_error() : "");
        if (grc != GS_OK) slices.close();
    }
    void close() {
        slices.close();
        feeds.close();
    }
};

struct TextJob {
    MatchCtx &c;
    std::string path;
    int bank;
    int64_t read_no;  // number of the next read of this file
    TextReader tr;
    // The reader's blocks into chunks of whole records; cut_.carry is what lies behind the last chunk and cut_.file_off where it
    // starts, for the device-inflated sources too (their leftover comes to the host once, at the end of the file).
    // FASTA files (AbstractFastqReader.doReadFasta): chunks are cut in front of a header line, the device finds the records
    // (gs_match_submit_fasta).  General FASTQ (sequence / quality over several lines): chunks of whole lines that start at a record's
    // descriptor line; the device finds the records (gs_match_submit_fastq_ml) and says how much of the chunk they cover, the rest is
    // carried into the next one.  A FASTQ file whose first chunk is not four-line FASTQ is read again this way (finish()).
    ChunkCutter cut_;
    std::vector<TextChunk> chunks;
    int64_t reads_in_file = 0, first_ticket = -1, next_block = 0;
    int64_t base_tot[3] = {0, 0, 0}, tot[3] = {0, 0, 0};
    bool done = false;
    double t0 = 0;
    std::future<void> formatting;  // per-read outputs of the previous chunk on their way to the writers
    int64_t n_formatted = 0;
    int64_t held_ticket = -1, held_block = -1;
    bool fasta = false, general = false;
    bool gz_ = false;
    int readers_ = 2;
    // gzip input of four-line FASTQ inflated on the device (DeviceInflate): without per-read outputs the text never exists on the host,
    // with them (Kraken-style lines, filtered FASTQ) it comes back once per chunk, page-locked, for the writers.  What the device path
    // cannot take (a chunk the record scan refuses, the unterminated tail of the file) goes the usual way.
    DeviceInflate dev_;
    int64_t dev_tickets_[2] = {-1, -1};  // BGZF: the record scan's copy out of the feed's text
    int64_t gz_ticket_ = -1;             // whole stream: ... out of the batch's text
    PooledBuf dev_text_[2];              // the text of a chunk on the host, for the per-read writers

    int file_idx = 0;       // progress records: the file's index in the call, and the number of its first read
    int64_t file_base = 0;
    bool stopped_on_request = false;  // this job (or the pass that re-read its file, or its parser) stopped and published the record of that

    TextJob(MatchCtx &ctx, const std::string &p, int bank_, int64_t first_read_no, bool fasta_ = false, int file_idx_ = 0)
        : c(ctx), path(p), bank(bank_), read_no(first_read_no), fasta(fasta_), file_idx(file_idx_), file_base(first_read_no) {}
    ~TextJob() { abort(); }
    // stops the readers (after the writers of the last chunk are through with its block)
    void abort() {
        drain();
        release_held();
        release_gunzipper();  // (before the file is unmapped: its upload thread reads the mapping)
        tr.close();
        dev_.close();
    }
    // The device gunzipper goes back to its pool BEFORE tr.close() unmaps the file (GunzipSlices::close; finish() is reached
    // mid-stream by every refusal or fallback).  Its device text stays valid until the object is reopened.
    void release_gunzipper() {
        if (!dev_.whole()) return;
        gs_match_sync(c.run);  // (the record scan may still be copying out of its text)
        dev_.slices.close();
    }

    // the four-line FASTQ chunk that was just submitted: first read number, reads; its descriptor lines are fetched from the device
    int chunk_submitted(int64_t first_no, int64_t n_reads) {
        if (!c.track_desc()) return GS_OK;
        gs_run *run = c.run;
        return c.update_max_contig(first_no, n_reads, [run](const int64_t *recs, int32_t m, uint8_t *out, int32_t stride) {
            return gs_match_text_descriptors(run, recs, m, out, stride);
        });
    }

    // the same after a FASTA or general FASTQ chunk, whose text (n_lines whole lines) is still in host memory at `text`: the device
    // gives the record geometry -- the newline offsets, and for general FASTQ the class of every line, as a '@' can also begin a
    // quality line -- and the descriptor lines are taken from the text
    int chunk_submitted_general(int64_t first_no, int64_t n_reads, const uint8_t *text, int64_t n_lines, bool is_fasta) {
        if (!c.track_desc()) return GS_OK;
        gs_run *run = c.run;
        return c.update_max_contig(first_no, n_reads, [=](const int64_t *recs, int32_t m, uint8_t *out, int32_t stride) -> int {
            std::vector<uint32_t> nl((size_t)std::max<int64_t>(n_lines, 1));
            std::vector<uint8_t> cls((size_t)std::max<int64_t>(n_lines, 1));
            int err = gs_match_text_newlines(run, nl.data());
            if (!err && !is_fasta) err = gs_match_text_line_classes(run, cls.data());
            if (err) return err;
            auto line_start = [&nl](int64_t i) { return i ? (size_t)nl[(size_t)i - 1] + 1 : (size_t)0; };
            std::vector<int64_t> head;  // descriptor line of every record (as outputs_general finds them)
            for (int64_t i = 0; i < n_lines; i++)
                if (is_fasta ? text[line_start(i)] == '>' && nl[(size_t)i] > line_start(i) : cls[(size_t)i] == 1) head.push_back(i);
            if ((int64_t)head.size() != n_reads) return hfail(GS_E_INVALID, "text chunk: the descriptor lines do not match the device's record count");
            for (int32_t j = 0; j < m; j++) {
                const int64_t h = head[(size_t)recs[j]];
                const size_t d0 = line_start(h), len = std::min<size_t>((size_t)nl[(size_t)h] - d0, (size_t)stride - 1);
                memcpy(out + (size_t)j * (size_t)stride, text + d0, len);
                out[(size_t)j * (size_t)stride + len] = 0;
            }
            return GS_OK;
        });
    }

    // Per-read outputs of a four-line chunk made on the device: the reads matchRead returned true for (afterMatch,
    // FastqKMerMatcher.java:304-307) are gathered there, the Kraken-style lines (:308-314) are written there behind the segments kernel,
    // and -- for a .gz file -- both are compressed there; the chunk's text, its newline offsets and its segments never come to the host.
    // GS_DEVICE_KRAKEN=0 takes the lines, and with them the filtered file, back to the host formatter.
    bool device_filtered() const { return device_output() && c.filtered.active() && (!c.kraken.active() || device_kraken()); }
    bool device_lines() const { return c.kraken.active() && device_kraken(); }
    bool device_per_read() const { return device_filtered() || device_lines(); }
    int dev_err_ = GS_OK;
    // after the chunk's flags are in (check_refusal has synchronised): gather and write the lines now, compress / fetch / write on a
    // thread of its own
    // records: the chunk is FASTA or general FASTQ (gs_match_compact_records / gs_match_kraken_records)
    int emit_device(bool records = false) {
        const int set = (int)(n_formatted & 1);
        const uint8_t *d = nullptr, *kd = nullptr;
        int64_t nb = 0, nr = 0, knb = 0, knl = 0;
        int err = GS_OK;
        if (c.filtered.active())
            err = records ? gs_match_compact_records(c.run, c.opts->with_probs != 0, set, &d, &nb, &nr)
                          : gs_match_compact_text(c.run, c.opts->with_probs != 0, set, &d, &nb, &nr);
        if (!err && c.kraken.active()) {
            if (!c.taxids_on_device) err = gs_match_set_taxids(c.run, c.opts->taxids);
            c.taxids_on_device = !err;
            if (!err)
                err = records ? gs_match_kraken_records(c.run, c.opts->write_all != 0, set, &kd, &knb, &knl)
                              : gs_match_kraken_text(c.run, c.opts->write_all != 0, set, &kd, &knb, &knl);
            if (!err && !records) g_kraken_device_chunks.fetch_add(1);
        }
        if (err) return err;
        if (records) g_record_device_chunks.fetch_add(1);
        c.filtered_reads += nr;
        drain();  // one chunk at a time: output order
        if (dev_err_) return dev_err_;
        n_formatted++;
        auto job = [this, set, d, nb, kd, knb] {
            int e = c.filtered_dev.emit(set, d, nb);
            if (!e) e = c.kraken_dev.emit(set, kd, knb);
            if (e) dev_err_ = e;
        };
        run_behind(formatting, job);
        return GS_OK;
    }

    int open(bool gzip, int readers) {
        size_t block;
        reader_shape(gzip, &block, &readers);
        t0 = now_s();
        gz_ = gzip;
        readers_ = readers;
        cut_.mode = general ? ChunkCutter::GENERAL : (fasta ? ChunkCutter::FASTA : ChunkCutter::FOUR_LINE);
        int err = tr.open(path, block, readers, gzip);
        if (!err) err = gs_match_text_select(c.run, bank);
        int64_t failed = -1, bad = -1;
        if (!err) err = gs_match_text_status(c.run, &failed, &bad, base_tot);  // totals this bank has seen before
        int device = 0;
        // (writers behind this job: a small first batch, so that they start after 10 ms and not after the 27 a full batch takes)
        if (!err && gzip && !fasta && !general && gs_match_get_device(c.run, &device) == GS_OK)
            dev_.open(tr.map, tr.map_len, device, (c.filtered.active() || c.kraken.active()) ? gunzip_first_span() : gunzip_first_span_match());
        if (!err && c.filtered.active() && gs_match_get_device(c.run, &device) == GS_OK) c.filtered_dev.begin(&c.filtered, device);
        if (!err && c.kraken.active() && gs_match_get_device(c.run, &device) == GS_OK) c.kraken_dev.begin(&c.kraken, device);
        if (!err && !dev_.bgzf() && !dev_.whole()) tr.start();
        return err;
    }

    // text per chunk of a device-inflated source (GS_HOST_BGZF_TEXT): a wave inflates a member in ~6 ms whatever else runs, so the
    // rate is the number of members under way -- 512 MiB are ~8000 members, two rounds over the device's wave slots; with writers
    // behind it a chunk is 128 MiB of text: they start four times earlier (as filter_bgzf_file)
    int64_t device_text_target() const {
        const bool per_read = c.filtered.active() || c.kraken.active();
        return per_read && !getenv("GS_HOST_BGZF_TEXT") ? ((int64_t)128 << 20) : bgzf_text_target();
    }
    void fall_back(int64_t *fallback_off, int64_t *fallback_reads) const {
        *fallback_off = cut_.file_off;
        *fallback_reads = reads_in_file;
    }

    // A four-line chunk whose text lies on the device, through the match kernel.  With per-read outputs the writers need the chunk's
    // results and its text: class / flags come to host arrays (GS_MEM_DEVICE_TEXT), fetch_text(dst) brings the text while the match
    // kernel runs, then the chunk is formatted on a thread of its own.  Without them the record scan takes its own copy of the text
    // (device to device): *scan_ticket, the caller's, says when that copy is through.
    int device_chunk(const DevText &t, const std::function<int(uint8_t *)> &fetch_text, int64_t *scan_ticket, int64_t *fallback_off, int64_t *fallback_reads) {
        const int64_t n_chunk = t.n_lines >> 2, first_no = read_no + reads_in_file;
        int64_t ticket = -1;
        if (!(c.filtered.active() || c.kraken.active())) {
            int err = gs_match_submit_text(c.run, t.text, t.n_bytes, t.n_lines, GS_MEM_DEVICE, first_no, nullptr, nullptr, &ticket);
            if (!err) err = chunk_submitted(first_no, n_chunk);
            if (err) return err;
            *scan_ticket = ticket;
            if (first_ticket < 0) first_ticket = ticket;
            chunks.push_back({cut_.file_off, reads_in_file, ticket});
            reads_in_file += n_chunk;
            cut_.file_off += t.n_bytes;
            return chunks.size() == 1 || (chunks.size() & 15) == 0 ? check_refusal(fallback_off, fallback_reads) : (int)GS_OK;
        }
        MatchCtx::Results &rs = c.res[n_formatted & 1];  // (the set of the chunk before last: its writers are done)
        PooledBuf &tb = dev_text_[n_formatted & 1];
        const bool dev_f = device_per_read();
        int err = rs.cls.resize((size_t)n_chunk);
        if (!err) err = rs.flags.resize((size_t)n_chunk);
        if (!err && !dev_f) err = tb.need((size_t)t.n_bytes);
        if (!err) err = gs_match_submit_text(c.run, t.text, t.n_bytes, t.n_lines, GS_MEM_DEVICE_TEXT, first_no, rs.cls.data(), rs.flags.data(), &ticket);
        if (!err) err = chunk_submitted(first_no, n_chunk);
        if (!err && !dev_f) err = fetch_text(static_cast<uint8_t *>(tb.p));
        if (err) return err;
        chunks.push_back({cut_.file_off, reads_in_file, ticket});
        err = check_refusal(fallback_off, fallback_reads);  // (synchronises: the results are needed now)
        if (!err && *fallback_off < 0 && !dev_f) err = fetch_chunk_results(rs, n_chunk);
        if (err || *fallback_off >= 0) {
            chunks.pop_back();
            return err;
        }
        if (first_ticket < 0) first_ticket = ticket;
        reads_in_file += n_chunk;
        cut_.file_off += t.n_bytes;
        if (dev_f) return emit_device();
        drain();  // one chunk at a time: output order, and the other result set becomes free
        n_formatted++;
        const uint8_t *h_text = static_cast<const uint8_t *>(tb.p);
        run_behind(formatting, [this, &rs, h_text, n_chunk] { format_chunk(rs, h_text, n_chunk, -1); });
        return GS_OK;
    }

    // the next slice of the device text: whole four-line records up to the chunk size, the leftover of the last slice to the host
    int step_gunzip(int *err_out) {
        int64_t fallback_off = -1, fallback_reads = 0;
        static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
        const double ts0 = now_s();
        DevText t;
        bool refused = false;
        // (the scan's copy out of a batch's text must be through before the text is replaced)
        int err = dev_.slices.next(device_text_target(), path, [this] {
            const int e = gz_ticket_ >= 0 ? gs_match_text_wait_copy(c.run, gz_ticket_) : (int)GS_OK;
            gz_ticket_ = -1;
            return e;
        }, &t, &refused);
        const double ts1 = now_s();
        if (!err) err = gs_match_text_select(c.run, bank);
        if (!err && (refused || t.stuck))
            fall_back(&fallback_off, &fallback_reads);
        else if (!err && t.n_lines > 0) {
            GunzipSlices &sl = dev_.slices;
            err = device_chunk(t, [&sl, &t](uint8_t *dst) { return sl.fetch_text(t, dst); }, &gz_ticket_, &fallback_off, &fallback_reads);
        }
        const double ts2 = now_s();
        if (err || t.last || fallback_off >= 0) {
            if (!err && fallback_off < 0) err = dev_.slices.fetch_leftover(cut_.carry);  // what is left behind the last whole record
            err = finish(err, fallback_off, fallback_reads);
        }
        if (trace)
            fprintf(stderr, "gunzip slice: %lld bytes, %lld lines: cut (+ next batch) %.2f ms, submit %.2f ms, finish %.2f ms\n", (long long)t.n_bytes, (long long)t.n_lines,
                    (ts1 - ts0) * 1e3, (ts2 - ts1) * 1e3, (now_s() - ts2) * 1e3);
        *err_out = err;
        return 1;
    }

    // one run of members: inflate on the device, submit the whole records, carry the rest (on the device)
    int step_bgzf(int *err_out) {
        // The previous feed's text went to the device scan, which takes its own copy (device to device, a fraction of a
        // millisecond): that copy must be through before this feed runs -- the feed ends by moving its leftover into the OTHER
        // text buffer, which is the one the scan is copying from.
        int err = GS_OK;
        if (dev_tickets_[0] >= 0) {
            err = gs_match_text_wait_copy(c.run, dev_tickets_[0]);
            dev_tickets_[0] = -1;
        }
        int64_t fallback_off = -1, fallback_reads = 0;
        static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
        const double tt0 = now_s();
        BgzfFeeds &fd = dev_.feeds;
        DevText t;
        if (!err) err = fd.next(device_text_target(), path, &t);
        const double tt1 = now_s();
        if (!err) err = gs_match_text_select(c.run, bank);
        if (!err && t.n_lines > 0)
            err = device_chunk(t, [&fd, &t](uint8_t *dst) { return fd.fetch_text(dst, t.n_bytes); }, &dev_tickets_[0], &fallback_off, &fallback_reads);
        else if (!err && t.stuck)
            fall_back(&fallback_off, &fallback_reads);
        if (trace)
            fprintf(stderr, "bgzf feed %lld: members up to %zu, feed %.2f ms, submit+check %.2f ms, %lld bytes %lld lines tail %lld\n", (long long)fd.n_feeds, fd.next_member,
                    (tt1 - tt0) * 1e3, (now_s() - tt1) * 1e3, (long long)t.n_bytes, (long long)t.n_lines, (long long)fd.tail);
        if (err || t.last || fallback_off >= 0) {
            if (!err && fallback_off < 0) err = fd.fetch_tail(cut_.carry);  // what is left behind the last whole record
            for (int q = 0; q < 2; q++)
                if (dev_tickets_[q] >= 0) {
                    const int e2 = gs_match_text_wait_copy(c.run, dev_tickets_[q]);
                    if (!err) err = e2;
                    dev_tickets_[q] = -1;
                }
            err = finish(err, fallback_off, fallback_reads);
        }
        *err_out = err;
        return 1;
    }

    // 1: a block was handled, 0: none ready (blocking = false only); `done` is set when the file is through.  With a control attached
    // to the thread every block that leaves the file unfinished ends with a progress record and a look at the cancel flag.
    int step(bool blocking, int *err_out) {
        const int r = step_block(blocking, err_out);
        if (r > 0 && *err_out == GS_E_CANCELLED) stopped_on_request = true;  // (the file's end stopped: its parser, or the pass that re-read it)
        if (r > 0 && !*err_out && !done && trk().on()) {
            int64_t pos = cut_.file_off;
            bool text_pos = gz_;
            if (dev_.bgzf()) {  // (the members say where they lie in the file)
                const BgzfFeeds &fd = dev_.feeds;
                pos = fd.next_member < fd.members.size() ? fd.members[fd.next_member].payload_offset : (int64_t)tr.map_len;
                text_pos = false;
            }
            if (trk().chunk(file_idx, pos, text_pos, read_no - file_base + reads_in_file)) *err_out = stop_on_request();
        }
        return r;
    }

    // A stop on request: nothing more is submitted.  The writers of the last chunk finish, the copies out of the held block and out of
    // device text complete, every chunk of the run completes (gs_match_sync) and is counted -- a chunk the device refused, and those
    // behind it, never reached the state: the file's prefix ends in front of it.  The record of the stop is published, and only then
    // do the blocks go back to their readers, the readers stop and the device decoders return to their pools.
    int stop_on_request() {
        done = true;
        stopped_on_request = true;
        drain();
        int err = dev_err_;
        auto keep = [&err](int e) {
            if (!err) err = e;
        };
        if (held_ticket >= 0) keep(gs_match_text_wait_copy(c.run, held_ticket));
        for (int q = 0; q < 2; q++)
            if (dev_tickets_[q] >= 0) {
                keep(gs_match_text_wait_copy(c.run, dev_tickets_[q]));
                dev_tickets_[q] = -1;
            }
        if (gz_ticket_ >= 0) keep(gs_match_text_wait_copy(c.run, gz_ticket_));
        gz_ticket_ = -1;
        keep(gs_match_sync(c.run));
        keep(gs_match_text_select(c.run, bank));
        int64_t fallback_off = -1, fallback_reads = 0;
        if (!err) err = check_refusal(&fallback_off, &fallback_reads);  // also fetches the totals
        if (!err && fallback_off >= 0) {
            int64_t failed = -1, bad = -1;
            err = gs_match_text_status(c.run, &failed, &bad, tot);  // (read after the refusal: exactly the accepted chunks)
            reads_in_file = fallback_reads;
        }
        if (!err) {
            c.reads += tot[0] - base_tot[0];
            c.kmers += tot[1] - base_tot[1];
            c.bps += tot[2] - base_tot[2];
            read_no += reads_in_file;
            trk().stopped(file_idx, read_no - file_base);
        }
        release_held();
        release_gunzipper();
        tr.close();
        dev_.close();
        c.t_parse += now_s() - t0;
        return err ? err : cancelled_rc();
    }

    int step_block(bool blocking, int *err_out) {
        if (dev_.bgzf()) return step_bgzf(err_out);
        if (dev_.whole()) return step_gunzip(err_out);
        const int64_t i = next_block;
        if (!blocking && !tr.is_full(i)) return 0;
        TextSlot &sl = tr.wait_full(i);
        int64_t fallback_off = -1, fallback_reads = 0;
        const bool last = sl.eof;
        bool keep_block = false;
        int err = block_error(tr, sl, path);
        if (!err) err = gs_match_text_select(c.run, bank);
        if (!err) switch (cut_block(cut_, tr, sl)) {
            case ChunkCutter::ABSORBED: break;
            case ChunkCutter::FALLBACK: fall_back(&fallback_off, &fallback_reads); break;  // the general parser takes over
            case ChunkCutter::CHUNK:
                err = general ? chunk_general(&fallback_off, &fallback_reads)
                              : (fasta ? chunk_fasta(i, &keep_block, &fallback_off, &fallback_reads) : chunk_four_line(i, &keep_block, &fallback_off, &fallback_reads));
        }
        if (!keep_block) tr.release(i);  // (else: release_held or format_chunk releases it)
        next_block = i + 1;
        if (err || last || fallback_off >= 0) err = finish(err, fallback_off, fallback_reads);
        *err_out = err;
        return 1;
    }

    // the chunk of four-line FASTQ that cut_ has just made of block i
    int chunk_four_line(int64_t i, bool *keep_block, int64_t *fallback_off, int64_t *fallback_reads) {
        uint8_t *start = cut_.start;
        int64_t ticket = -1;
        bool format_it = false;
        const bool per_read = c.filtered.active() || c.kraken.active();
        const int64_t n_chunk = cut_.lines >> 2, first_no = read_no + reads_in_file;
        MatchCtx::Results &rs = c.res[n_formatted & 1];  // (the set of the chunk before last: its writers are done)
        int err = GS_OK;
        if (per_read) {
            err = rs.cls.resize((size_t)n_chunk);
            if (!err) err = rs.flags.resize((size_t)n_chunk);
        }
        if (!err)
            err = gs_match_submit_text(c.run, start, cut_.bytes, cut_.lines, GS_MEM_HOST, first_no, per_read ? rs.cls.data() : nullptr,
                                       per_read ? rs.flags.data() : nullptr, &ticket);
        if (!err) err = chunk_submitted(first_no, n_chunk);
        // (a plain filtered file alone: formatted from the reader's block, which is here anyway; the lines need the segments, which
        // are on the device)
        const bool dev_f = per_read && device_per_read() && (device_lines() || c.filtered.gzip());
        if (!err && per_read) {  // the writers need this chunk's results
            chunks.push_back({cut_.file_off, reads_in_file, ticket});
            err = check_refusal(fallback_off, fallback_reads);
            chunks.pop_back();
            if (!err && *fallback_off < 0 && !dev_f) err = fetch_chunk_results(rs, n_chunk);
            format_it = !err && *fallback_off < 0 && !dev_f;
            if (!err && *fallback_off < 0 && dev_f) err = emit_device();
        }
        if (!err && *fallback_off < 0) {
            if (first_ticket < 0) first_ticket = ticket;
            chunks.push_back({cut_.file_off, reads_in_file, ticket});
            reads_in_file += n_chunk;
            cut_.commit();
            if (format_it) {
                err = gs_match_text_wait_copy(c.run, ticket);  // (the writers hand the block back, below)
            } else {
                // the pinned block goes back to its reader when its copy is through: looked at one chunk later,
                // so that this thread is already submitting the next copy while this one runs
                err = release_held();
                held_ticket = ticket;
                held_block = i;
                *keep_block = true;
            }
        }
        if (format_it && !err) {
            // (only now: the block returns to its reader when the writers are through with it, and the
            // carry above had to be taken out first)
            drain();  // one chunk at a time: output order, and the other result set becomes free
            n_formatted++;
            *keep_block = true;
            run_behind(formatting, [this, &rs, start, n_chunk, i] { format_chunk(rs, start, n_chunk, i); });
        }
        // a file that is not four-line FASTQ fails in its first chunk: look early, then now and again
        if (!err && *fallback_off < 0 && !per_read && (chunks.size() == 1 || (chunks.size() & 15) == 0)) err = check_refusal(fallback_off, fallback_reads);
        return err;
    }

    // The FASTA form: the chunk ends in front of the block's last header line (everything up to there is whole records), the rest
    // is carried into the next block.  Headers and newlines were counted on the host (ChunkCutter), the device checks the counts.
    int chunk_fasta(int64_t i, bool *keep_block, int64_t *fallback_off, int64_t *fallback_reads) {
        const int64_t records = cut_.records, first_no = read_no + reads_in_file;
        int64_t ticket = -1;
        int err = GS_OK;
        if (cut_.bytes > 0) {
            const bool kr = c.kraken.active() || c.filtered.active();
            MatchCtx::Results &rs = c.res[0];
            if (kr) {
                err = rs.cls.resize((size_t)std::max<int64_t>(records, 1));
                if (!err) err = rs.flags.resize((size_t)std::max<int64_t>(records, 1));
            }
            if (!err)
                err = gs_match_submit_fasta(c.run, cut_.start, cut_.bytes, cut_.lines, records, GS_MEM_HOST, first_no, kr ? rs.cls.data() : nullptr,
                                            kr ? rs.flags.data() : nullptr, &ticket);
            if (!err) err = chunk_submitted_general(first_no, records, cut_.start, cut_.lines, true);
            if (!err && kr && records > 0) {  // the per-read outputs of this chunk's records, before the block goes back
                chunks.push_back({cut_.file_off, reads_in_file, ticket});
                err = check_refusal(fallback_off, fallback_reads);
                chunks.pop_back();
                if (!err && *fallback_off < 0) err = outputs_general(rs, cut_.start, cut_.lines, records, true);
            }
        }
        if (!err && *fallback_off < 0) {
            if (ticket >= 0) {
                if (first_ticket < 0) first_ticket = ticket;
                chunks.push_back({cut_.file_off, reads_in_file, ticket});
            }
            reads_in_file += records;
            cut_.commit();
            if (ticket >= 0) {
                err = release_held();
                held_ticket = ticket;
                held_block = i;
                *keep_block = true;
            }
        }
        if (!err && *fallback_off < 0 && (chunks.size() == 1 || (chunks.size() & 15) == 0)) err = check_refusal(fallback_off, fallback_reads);
        return err;
    }

    // The general form: everything up to the block's last newline goes to the device together with what the last chunk left over;
    // the device reports how many records END in it and how many bytes they cover.
    int chunk_general(int64_t *fallback_off, int64_t *fallback_reads) {
        const int64_t first_no = read_no + reads_in_file;
        int64_t n_rec = 0, used = 0, used_lines = 0, ticket = -1;
        const bool kr = c.kraken.active() || c.filtered.active();
        MatchCtx::Results &rs = c.res[0];
        int err = GS_OK;
        if (kr) {
            err = rs.cls.resize((size_t)(cut_.lines / 4 + 2));
            if (!err) err = rs.flags.resize((size_t)(cut_.lines / 4 + 2));
        }
        if (!err)
            err = gs_match_submit_fastq_ml(c.run, cut_.start, cut_.bytes, cut_.lines, GS_MEM_HOST, first_no, kr ? rs.cls.data() : nullptr, kr ? rs.flags.data() : nullptr,
                                           &n_rec, &used, &used_lines, &ticket);
        if (!err && n_rec > 0) err = chunk_submitted_general(first_no, n_rec, cut_.start, used_lines, false);
        if (!err && kr && n_rec > 0) err = outputs_general(rs, cut_.start, used_lines, n_rec, false);
        if (!err && n_rec < 0) {  // refused (NUL byte, a record of thousands of lines): the general parser from here
            err = gs_match_text_clear_error(c.run);
            fall_back(fallback_off, fallback_reads);
        } else if (!err) {
            g_ml_chunks.fetch_add(1);
            if (first_ticket < 0) first_ticket = ticket;
            reads_in_file += n_rec;
            cut_.commit(used, used_lines);  // (the text has been copied)
        }
        return err;
    }

    // Per-read outputs of a FASTA or general FASTQ chunk that has just been matched.  Record geometry: the newline offsets from the
    // device and a class per line (1 descriptor, 2 sequence, 0 '+' / quality) -- from the device for general FASTQ, by the
    // first byte for FASTA.  Kraken-style lines (MatcherReadEntry.writeMatchDetails, :723-756): descriptor up to the first blank
    // without its first character, class, length, runs.  Filtered FASTQ: append_general_record.
    // On the device under the condition of the four-line chunks (device_filtered / device_lines; GS_DEVICE_RECORDS=0: here).
    int outputs_general(MatchCtx::Results &rs, const uint8_t *text, int64_t n_lines, int64_t n_records, bool is_fasta) {
        if (device_records() && device_per_read() && (device_lines() || c.filtered.gzip())) return emit_device(true);
        std::vector<uint64_t> bounds((size_t)n_records + 1);
        std::vector<uint8_t> cls((size_t)std::max<int64_t>(n_lines, 1));
        int err = gs_match_text_read_bounds(c.run, bounds.data());  // (waits for the chunk: cls / flags are complete)
        if (!err) err = rs.nl.resize((size_t)std::max<int64_t>(n_lines, 1));
        if (!err) err = gs_match_text_newlines(c.run, rs.nl.data());
        if (!err && !is_fasta) err = gs_match_text_line_classes(c.run, cls.data());
        if (!err && c.kraken.active()) {
            err = rs.seg_off.resize((size_t)n_records + 1);
            if (!err) err = gs_match_segments_text(c.run, rs.seg_off.data());
            if (!err) err = rs.seg_code.resize((size_t)rs.seg_off[(size_t)n_records]);
            if (!err) err = rs.seg_start.resize((size_t)rs.seg_off[(size_t)n_records]);
            if (!err) err = gs_match_segments_fetch(c.run, rs.seg_code.data(), rs.seg_start.data());
        }
        if (err) return err;
        const uint32_t *nl = rs.nl.p;
        auto line_start = [nl](int64_t i) { return i ? (size_t)nl[i - 1] + 1 : (size_t)0; };
        if (is_fasta)
            for (int64_t i = 0; i < n_lines; i++) cls[(size_t)i] = text[line_start(i)] == '>' && nl[i] > line_start(i) ? 1 : 2;
        std::vector<int64_t> head;  // descriptor line of every record, + n_lines
        head.reserve((size_t)n_records + 1);
        for (int64_t i = 0; i < n_lines; i++)
            if (cls[(size_t)i] == 1) head.push_back(i);
        if ((int64_t)head.size() != n_records) return hfail(GS_E_INVALID, "text chunk: the descriptor lines do not match the device's record count");
        head.push_back(n_lines);
        std::vector<FormatPart> parts((size_t)c.pool.threads());
        MatchCtx &cc = c;
        const bool probs = c.opts->with_probs != 0 && !is_fasta;
        c.pool.run(n_records, [&](int t, int64_t lo, int64_t hi) {
            FormatPart &p = parts[(size_t)t];
            p.filtered = cc.filtered.take();
            p.kraken = cc.kraken.take();
            for (int64_t r = lo; r < hi; r++) {
                const int64_t h = head[(size_t)r], next = head[(size_t)r + 1];
                const size_t d0 = line_start(h), dlen = (size_t)nl[h] - d0;
                const int64_t L = (int64_t)(bounds[(size_t)r + 1] - bounds[(size_t)r]);
                if (cc.filtered.active() && (rs.flags[(size_t)r] & GS_F_RETURNED)) {
                    append_general_record(p.filtered, text, nl, cls.data(), h, next, L, is_fasta, probs);
                    p.n_filtered++;
                }
                if (cc.kraken.active()) kraken_line(cc, rs, p.kraken, text + d0, dlen, L, r);
            }
            p.pack(cc.kraken, cc.filtered);
        });
        drain();  // (a chunk whose device text is still on its way out comes first)
        write_parts(c, parts);
        return GS_OK;
    }

private:
    // filtered FASTQ (afterMatch, :304-307) and Kraken-style lines (:723-756) of the chunk that was just matched, from
    // the raw block: the device returns the record geometry (newline offsets) and the segments (fetch_chunk_results,
    // on the submitting thread), the lines are formatted and handed to the writers on a thread of their own
    // (format_chunk) while the next chunk is on the device; the chunk's block goes back to its reader afterwards
    int fetch_chunk_results(MatchCtx::Results &rs, int64_t n) {
        int err = rs.nl.resize((size_t)n * 4);
        if (!err) err = gs_match_text_newlines(c.run, rs.nl.data());
        if (!err && c.kraken.active()) {
            err = rs.seg_off.resize((size_t)n + 1);
            if (!err) err = gs_match_segments_text(c.run, rs.seg_off.data());
            if (!err) err = rs.seg_code.resize((size_t)rs.seg_off[(size_t)n]);
            if (!err) err = rs.seg_start.resize((size_t)rs.seg_off[(size_t)n]);
            if (!err) err = gs_match_segments_fetch(c.run, rs.seg_code.data(), rs.seg_start.data());
        }
        return err;
    }

    void format_chunk(const MatchCtx::Results &rs, const uint8_t *text, int64_t n, int64_t block) {
        std::vector<FormatPart> parts((size_t)c.pool.threads());
        MatchCtx &cc = c;
        const uint32_t *nl = rs.nl.p;
        c.pool.run(n, [&cc, &rs, &parts, text, nl](int t, int64_t lo, int64_t hi) {
            FormatPart &p = parts[(size_t)t];
            p.filtered = cc.filtered.take();
            p.kraken = cc.kraken.take();
            for (int64_t r = lo; r < hi; r++) {
                if (cc.filtered.active() && (rs.flags[(size_t)r] & GS_F_RETURNED)) {
                    append_text_record(p.filtered, text, nl, r, cc.opts->with_probs != 0);
                    p.n_filtered++;
                }
                if (cc.kraken.active()) {
                    const size_t d0 = r == 0 ? 0 : (size_t)nl[4 * r - 1] + 1, d1 = nl[4 * r];
                    kraken_line(cc, rs, p.kraken, text + d0, d1 - d0, (int64_t)nl[4 * r + 1] - (int64_t)d1 - 1, r);
                }
            }
            p.pack(cc.kraken, cc.filtered);
        });
        write_parts(c, parts);
        if (block >= 0) tr.release(block);  // (-1: the text was not a reader's block -- device-inflated input)
    }

    // waits for the chunk that is being formatted (its result set and its block are free afterwards)
    void drain() {
        if (formatting.valid()) formatting.get();
    }
    // the block whose copy to the device was still running when the thread went on
    int release_held() {
        if (held_ticket < 0) return GS_OK;
        const int err = gs_match_text_wait_copy(c.run, held_ticket);
        tr.release(held_block);
        held_ticket = -1;
        return err;
    }

    int check_refusal(int64_t *fallback_off, int64_t *fallback_reads) {
        int64_t failed = -1, bad = -1;
        int err = gs_match_text_status(c.run, &failed, &bad, tot);
        if (err || failed < 0) return err;
        for (const TextChunk &ch : chunks)
            if (ch.ticket == failed) {
                *fallback_off = ch.file_off;
                *fallback_reads = ch.reads_before;
            }
        return gs_match_text_clear_error(c.run);
    }

    int finish(int err, int64_t fallback_off, int64_t fallback_reads) {
        done = true;
        drain();
        if (!err) err = dev_err_;
        const int held_err = release_held();  // (the blocks return to the pool in close(): no copy may still read them)
        if (!err) err = held_err;
        release_gunzipper();  // (parks the upload thread: it reads the mapping that close() removes)
        tr.close();
        c.t_parse += now_s() - t0;
        if (err) return err;
        err = gs_match_text_select(c.run, bank);
        if (!err && fallback_off < 0) err = check_refusal(&fallback_off, &fallback_reads);  // also fetches the final totals
        if (err) return err;
        if (fallback_off >= 0) {  // `tot` was read after the refusal: it holds exactly the accepted chunks
            int64_t failed = -1, bad = -1;
            err = gs_match_text_status(c.run, &failed, &bad, tot);
            if (err) return err;
        }
        c.reads += tot[0] - base_tot[0];
        c.kmers += tot[1] - base_tot[1];
        c.bps += tot[2] - base_tot[2];
        if (fallback_off >= 0) {
            read_no += fallback_reads;
            // a FASTQ file that is not four lines per record from its very first chunk: once more with the records found on the
            // device (GS_HOST_ML=0: straight to the reference-exact parser, which also takes over whatever that pass refuses)
            bool ml = fallback_off == 0 && fallback_reads == 0 && !fasta && !general;
            if (const char *e = getenv("GS_HOST_ML")) ml = ml && atoi(e) != 0;
            c.prog_file = file_idx;
            c.prog_base = file_base;
            if (ml) {
                TextJob g(c, path, bank, read_no, false, file_idx);
                g.file_base = file_base;
                g.general = true;
                int gerr = g.open(gz_, readers_);
                while (!gerr && !g.done) g.step(true, &gerr);
                if (!g.done) g.abort();
                read_no = g.read_no;
                return gerr;
            }
            return parsed_source(c, path, fallback_off, nullptr, 0, read_no);
        }
        read_no += reads_in_file;
        c.prog_file = file_idx;
        c.prog_base = file_base;
        // what is left after the last whole four-line group (no final newline, truncated record): the general parser
        if (!cut_.carry.empty()) return parsed_source(c, std::string(), 0, cut_.carry.data(), cut_.carry.size(), read_no, fasta);
        return GS_OK;
    }
};

}  // namespace

namespace {

// the files of one runMatcher call into c.run (begin and finish are the caller's).  file_index (may be NULL): the
// position of each file in the global file order when several processes share the files of a run; read numbers are then
// (file_index << 32 | read in file).  reads_of_file[n_paths] receives the read counts, *composite says whether the
// max-contig read numbers of the run are in that (file, read) form.
int run_files(MatchCtx &c, const char *const *paths, int n_paths, const int32_t *file_index, std::vector<int64_t> &reads_of_file_out,
              bool *composite, bool allow_side_by_side = true) {
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    int err = GS_OK;
    std::vector<int> kind((size_t)n_paths, 0);
    int n_gzip = 0;
    for (int i = 0; i < n_paths; i++) {
        kind[(size_t)i] = fast ? text_path_kind(paths[i]) : 0;
        n_gzip += kind[(size_t)i] == 2 || kind[(size_t)i] == 4;
    }
    const int default_readers = (int)std::min<unsigned>(8, std::max<unsigned>(2, std::thread::hardware_concurrency() / 2));
    // one gzip file at a time: its inflating threads are all the parallelism there is (measured on the MI355X box,
    // tools/gz_threads_sweep.py: 8 threads 1.7 Gbp/s, 12 2.3, 16 2.9, 24 3.3)
    const int gzip_threads = (int)std::min<unsigned>(16, std::max<unsigned>(2, std::thread::hardware_concurrency() / 2));
    // Several gzip files: each is bound by its single inflating thread, so they are read side by side (up to 8 at a
    // time).  The read numbers of file f then start at f << 32, which keeps "first read in file order" (the max-contig
    // tie-break) intact; the column is converted back to running read numbers at the end.
    // (per-read outputs follow the read order: one file after the other)
    bool side_by_side = n_gzip >= 2 && n_paths <= 256 && !c.filtered.active() && !c.kraken.active();
    if (const char *e = getenv("GS_HOST_PARALLEL_FILES")) side_by_side = side_by_side && atoi(e) != 0;
    side_by_side = side_by_side && allow_side_by_side;
    if (file_index) side_by_side = true;  // read numbers are (file << 32 | read): the files are independent anyway
    std::vector<int64_t> reads_of_file((size_t)n_paths, 0);
    Tracker &tk = trk();
    if (!side_by_side) {
        int64_t read_no = 0;
        for (int i = 0; i < n_paths && !err; i++) {
            const std::string path(paths[i]);
            const int64_t first_no = read_no;
            if (tk.file_start(i)) {
                tk.stopped(i, 0);
                err = cancelled_rc();
                break;
            }
            if (kind[(size_t)i]) {
                const bool gz = kind[(size_t)i] == 2 || kind[(size_t)i] == 4;
                TextJob job(c, path, 0, read_no, kind[(size_t)i] >= 3, i);
                err = job.open(gz, gz ? gzip_threads : default_readers);
                while (!err && !job.done) job.step(true, &err);
                if (!job.done) job.abort();
                read_no = job.read_no;
            } else {
                c.prog_file = i;
                c.prog_base = read_no;
                err = parsed_source(c, path, 0, nullptr, 0, read_no);
            }
            reads_of_file[(size_t)i] = read_no - first_no;
            if (!err && tk.file_end(i, read_no - first_no)) err = cancelled_rc();
        }
    } else {
        std::vector<std::unique_ptr<TextJob>> active;
        std::vector<int> file_of;
        int next = 0;
        while (!err && (next < n_paths || !active.empty())) {
            while (!err && next < n_paths && (int)active.size() < 8) {
                const int64_t base = (int64_t)(file_index ? file_index[next] : next) << 32;
                if (tk.file_start(next)) {
                    tk.stopped(next, 0);
                    err = cancelled_rc();
                    break;
                }
                if (kind[(size_t)next]) {
                    int bank = 0;  // a free bank
                    for (;; bank++) {
                        bool used = false;
                        for (auto &j : active) used = used || j->bank == bank;
                        if (!used) break;
                    }
                    auto job = std::make_unique<TextJob>(c, std::string(paths[next]), bank, base, kind[(size_t)next] >= 3, next);
                    err = job->open(kind[(size_t)next] == 2 || kind[(size_t)next] == 4, std::max(2, 2 * default_readers / std::min(n_paths, 8)));
                    active.push_back(std::move(job));
                    file_of.push_back(next);
                } else {  // FASTA etc.: the general parser, on its own
                    int64_t read_no = base;
                    c.prog_file = next;
                    c.prog_base = base;
                    err = parsed_source(c, std::string(paths[next]), 0, nullptr, 0, read_no);
                    reads_of_file[(size_t)next] = read_no - base;
                    if (!err && tk.file_end(next, read_no - base)) err = cancelled_rc();
                }
                next++;
            }
            bool progressed = false;
            for (size_t j = 0; j < active.size() && !err; j++) progressed = active[j]->step(false, &err) > 0 || progressed;
            for (size_t j = 0; j < active.size();) {
                if (active[j]->done) {
                    reads_of_file[(size_t)file_of[j]] = active[j]->read_no - ((int64_t)(file_index ? file_index[file_of[j]] : file_of[j]) << 32);
                    if (reads_of_file[(size_t)file_of[j]] >= ((int64_t)1 << 32) && !err)
                        err = hfail(GS_E_UNSUPPORTED, "more than 2^32 reads in one of several files read side by side (set GS_HOST_PARALLEL_FILES=0)");
                    if (!err && tk.file_end(file_of[j], reads_of_file[(size_t)file_of[j]])) err = cancelled_rc();
                    // a file that went through its last block in the sweep in which another file saw the flag: all of it is in
                    // the state, and the records say so (a job that stopped itself has published the record of its stop)
                    else if (err == GS_E_CANCELLED && !active[j]->stopped_on_request)
                        tk.file_end(file_of[j], reads_of_file[(size_t)file_of[j]], false);
                    active.erase(active.begin() + (long)j);
                    file_of.erase(file_of.begin() + (long)j);
                } else
                    j++;
            }
            if (!progressed && !active.empty()) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        // a stop on request: the files that were still being read stop the same way, each with the record of its own prefix
        for (size_t j = 0; j < active.size(); j++) {
            if (err == GS_E_CANCELLED && !active[j]->done) {
                const int e = active[j]->stop_on_request();
                if (e != GS_E_CANCELLED) err = e;
                reads_of_file[(size_t)file_of[j]] = active[j]->read_no - active[j]->file_base;
            }
            active[j]->abort();
        }
    }
    if (!err && tk.close()) err = cancelled_rc();
    reads_of_file_out = reads_of_file;
    *composite = side_by_side;
    return err;
}

}  // namespace

extern "C" int gs_host_match_into(gs_run *run, gs_db *db, const char *const *paths, int n_paths, const int32_t *file_index,
                                  int64_t *reads_of_file, gs_host_totals *totals);

extern "C" int gs_host_match_files(gs_db *db, const gs_match_cfg *cfg, const char *const *paths, int n_paths,
                                   const gs_host_match_opts *opts, int64_t *table, double *dtable,
                                   gs_host_totals *totals) try {
    if (!db || !cfg || !paths || n_paths < 0 || !table) return hfail(GS_E_INVALID, "NULL argument");
    MatchCtx c;
    int rc = gs_db_get_info(db, &c.info);
    if (rc) return rc;
    const gs_host_match_opts none{};
    if (!opts) opts = &none;
    c.opts = opts;
    if (opts->kraken_out_path && !opts->taxids) return hfail(GS_E_INVALID, "Kraken-style output needs the taxid strings");
    if (opts->kraken_out_path) {
        c.taxid_len.resize((size_t)c.info.n_values);
        for (int32_t v = 0; v < c.info.n_values; v++) {
            if (!opts->taxids[v]) return hfail(GS_E_INVALID, "Kraken-style output: a taxid string is NULL");
            c.taxid_len[(size_t)v] = (uint32_t)strlen(opts->taxids[v]);
            c.taxid_max = std::max(c.taxid_max, (size_t)c.taxid_len[(size_t)v]);
        }
    }
    if (c.track_desc()) memset(opts->max_contig_desc, 0, (size_t)c.info.n_values * (size_t)opts->max_contig_desc_stride);
    if (!c.filtered.open(opts->filtered_path) || !c.kraken.open(opts->kraken_out_path)) return hfail(GS_E_INVALID, "cannot open output file");
    const double t_begin = now_s();
    rc = gs_match_begin(&c.run, db, cfg);
    if (rc) return rc;
    const double t_start = now_s();
    std::vector<int64_t> reads_of_file;
    bool side_by_side = false;
    TrackerScope progress(paths, n_paths);
    int err = run_files(c, paths, n_paths, nullptr, reads_of_file, &side_by_side);
    const bool stopped = err == GS_E_CANCELLED;  // a stop on request: the table over the reads of the last records, then the code
    if (stopped) err = GS_OK;
    const double t_files = now_s();
    if (!err) err = gs_match_finish(c.run, table, dtable);
    const double t_fin = now_s();
    if (!err && side_by_side) {  // (file << 32 | read in file) -> running read number over the files in order
        std::vector<int64_t> before((size_t)n_paths + 1, 0);
        for (int i = 0; i < n_paths; i++) before[(size_t)i + 1] = before[(size_t)i] + reads_of_file[(size_t)i];
        for (int32_t v = 0; v < c.info.n_values; v++) {
            int64_t &x = table[(size_t)v * GS_N_COLS + GS_C_MAX_CONTIG_READ_NO];
            if (x >= 0) x = before[(size_t)(x >> 32)] + (x & 0xffffffffLL);
        }
    }
    gs_match_destroy(c.run);
    const bool wrote = c.filtered.close() & c.kraken.close();  // (both are flushed before the clock stops)
    if (!err) err = c.filtered_dev.late_err;
    if (!err) err = c.kraken_dev.late_err;
    if (getenv("GS_HOST_TRACE") != nullptr)
        fprintf(stderr, "match files: begin %.2f ms, files %.2f, finish %.2f, destroy + close %.2f\n", (t_start - t_begin) * 1e3, (t_files - t_start) * 1e3, (t_fin - t_files) * 1e3,
                (now_s() - t_fin) * 1e3);
    if (!err && !wrote) err = hfail(GS_E_IO, "write to an output file failed");
    if (totals) {
        totals->reads = c.reads;
        totals->kmers = c.kmers;
        totals->bps = c.bps;
        totals->filtered_reads = c.filtered_reads;
        totals->seconds_total = now_s() - t_start;
        totals->seconds_parse = c.t_parse;
        totals->seconds_gpu = c.t_gpu;
    }
    return !err && stopped ? cancelled_rc() : err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}


// runMatcher's body for a host that keeps its own run (begin / reset ... finish): the files into `run`, per-read outputs included
extern "C" int gs_host_match_run(gs_run *run, gs_db *db, const char *const *paths, int n_paths, const gs_host_match_opts *opts,
                                 gs_host_totals *totals) try {
    if (!run || !db || !paths || n_paths < 0) return hfail(GS_E_INVALID, "NULL argument");
    MatchCtx c;
    int rc = gs_db_get_info(db, &c.info);
    if (rc) return rc;
    const gs_host_match_opts none{};
    if (!opts) opts = &none;
    c.opts = opts;
    if (opts->kraken_out_path && !opts->taxids) return hfail(GS_E_INVALID, "Kraken-style output needs the taxid strings");
    if (opts->kraken_out_path) {
        c.taxid_len.resize((size_t)c.info.n_values);
        for (int32_t v = 0; v < c.info.n_values; v++) {
            if (!opts->taxids[v]) return hfail(GS_E_INVALID, "Kraken-style output: a taxid string is NULL");
            c.taxid_len[(size_t)v] = (uint32_t)strlen(opts->taxids[v]);
            c.taxid_max = std::max(c.taxid_max, (size_t)c.taxid_len[(size_t)v]);
        }
    }
    if (c.track_desc()) memset(opts->max_contig_desc, 0, (size_t)c.info.n_values * (size_t)opts->max_contig_desc_stride);
    if (!c.filtered.open(opts->filtered_path) || !c.kraken.open(opts->kraken_out_path)) return hfail(GS_E_INVALID, "cannot open output file");
    c.run = run;
    const double t_start = now_s();
    std::vector<int64_t> reads_of_file;
    bool composite = false;
    TrackerScope progress(paths, n_paths);
    int err = run_files(c, paths, n_paths, nullptr, reads_of_file, &composite, false);  // (one file after the other: running read numbers)
    const bool stopped = err == GS_E_CANCELLED;  // a stop on request: the outputs are closed as after a whole run, then the code
    if (stopped) err = GS_OK;
    if (!err) err = gs_match_sync(run);
    const bool wrote = c.filtered.close() & c.kraken.close();
    if (!err) err = c.filtered_dev.late_err;
    if (!err) err = c.kraken_dev.late_err;
    if (!err && !wrote) err = hfail(GS_E_IO, "write to an output file failed");
    if (totals) {
        totals->reads = c.reads;
        totals->kmers = c.kmers;
        totals->bps = c.bps;
        totals->filtered_reads = c.filtered_reads;
        totals->seconds_total = now_s() - t_start;
        totals->seconds_parse = c.t_parse;
        totals->seconds_gpu = c.t_gpu;
    }
    return !err && stopped ? cancelled_rc() : err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// runMatcher over the files of a sample on SEVERAL devices of this process: dbs[d] = a replica of the store on device d
// (the same arrays through gs_db_create, or the same store file).  File i goes to replica i % n_dbs; every replica has its
// own run and its own worker thread (reader pool, device text path, as gs_host_match_into); read numbers are
// (file << 32 | read), so that the max-contig tie-break keeps the file order; the runs are merged by gs_match_merge
// (kernels on one device, RCCL between devices) and finished once.  No per-read outputs (they would interleave).
extern "C" int gs_host_match_files_multi(gs_db *const *dbs, int n_dbs, const gs_match_cfg *cfg, const char *const *paths,
                                         int n_paths, int64_t *table, double *dtable, gs_host_totals *totals) try {
    if (!dbs || n_dbs < 1 || !cfg || !paths || n_paths < 0 || !table) return hfail(GS_E_INVALID, "NULL argument");
    if (n_paths > GS_HOST_MAX_FILE_INDEX) return hfail(GS_E_UNSUPPORTED, "at most 256 files per call");
    const double t_start = now_s();
    std::vector<gs_run *> runs((size_t)n_dbs, nullptr);
    int err = GS_OK;
    for (int d = 0; d < n_dbs && !err; d++) {
        if (!dbs[d]) err = hfail(GS_E_INVALID, "a store is NULL");
        if (!err) err = gs_match_begin(&runs[(size_t)d], dbs[d], cfg);
    }
    std::vector<std::vector<int32_t>> mine((size_t)n_dbs);
    for (int i = 0; i < n_paths; i++) mine[(size_t)(i % n_dbs)].push_back(i);
    std::vector<int64_t> reads_of_file((size_t)n_paths, 0);
    std::vector<gs_host_totals> tot((size_t)n_dbs);
    std::vector<int> rcs((size_t)n_dbs, GS_OK);
    std::vector<std::string> msgs((size_t)n_dbs);
    if (!err) {
        std::vector<std::thread> th;
        for (int d = 0; d < n_dbs; d++)
            th.emplace_back([&, d] {
                const std::vector<int32_t> &idx = mine[(size_t)d];
                if (idx.empty()) return;
                std::vector<const char *> p;
                for (int32_t i : idx) p.push_back(paths[i]);
                std::vector<int64_t> rof(idx.size(), 0);
                rcs[(size_t)d] = gs_host_match_into(runs[(size_t)d], dbs[d], p.data(), (int)p.size(), idx.data(), rof.data(), &tot[(size_t)d]);
                if (rcs[(size_t)d]) msgs[(size_t)d] = gs_host_last_error();  // (the message is per thread)
                for (size_t x = 0; x < idx.size(); x++) reads_of_file[(size_t)idx[x]] = rof[x];
            });
        for (auto &t : th) t.join();
        for (int d = 0; d < n_dbs && !err; d++)
            if (rcs[(size_t)d]) err = hfail(rcs[(size_t)d], msgs[(size_t)d]);
    }
    if (!err) err = gs_match_merge(runs.data(), n_dbs);
    if (!err) err = gs_match_finish(runs[0], table, dtable);
    if (!err) {  // (file << 32 | read in file) -> running read number over the files in order
        gs_db_info info{};
        gs_db_get_info(dbs[0], &info);
        std::vector<int64_t> before((size_t)n_paths + 1, 0);
        for (int i = 0; i < n_paths; i++) before[(size_t)i + 1] = before[(size_t)i] + reads_of_file[(size_t)i];
        for (int32_t v = 0; v < info.n_values; v++) {
            int64_t &x = table[(size_t)v * GS_N_COLS + GS_C_MAX_CONTIG_READ_NO];
            if (x >= 0) x = before[(size_t)(x >> 32)] + (x & 0xffffffffLL);
        }
    }
    for (gs_run *r : runs)
        if (r) gs_match_destroy(r);
    if (totals) {
        *totals = gs_host_totals{};
        for (const gs_host_totals &t : tot) {
            totals->reads += t.reads;
            totals->kmers += t.kmers;
            totals->bps += t.bps;
            totals->seconds_parse += t.seconds_parse;
            totals->seconds_gpu += t.seconds_gpu;
        }
        totals->seconds_total = now_s() - t_start;
    }
    return err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// The same, into a run the caller began and will finish: for one-process-per-GPU runs that share the files of a sample
// (genestrip_amd/distributed.py: match_files_sharded) -- every process takes some of the files, merges the device state
// of its run with the others (gs_match_device_state) and finishes.  file_index[n_paths] = position of each file in the
// global file order; the read numbers handed to the device are (file_index << 32 | read in file), reads_of_file[n_paths]
// receives the read counts (needed to turn the max-contig read numbers into running ones after the merge).
extern "C" int gs_host_match_into(gs_run *run, gs_db *db, const char *const *paths, int n_paths, const int32_t *file_index,
                                  int64_t *reads_of_file, gs_host_totals *totals) try {
    if (!run || !db || !paths || n_paths < 0 || !file_index || !reads_of_file) return hfail(GS_E_INVALID, "NULL argument");
    // the max-contig key keeps 40 bits of the read number (gs_kernels.hip: key_lo): 8 of them are the file, 32 the read
    for (int i = 0; i < n_paths; i++)
        if (file_index[i] < 0 || file_index[i] >= GS_HOST_MAX_FILE_INDEX)
            return hfail(GS_E_UNSUPPORTED, "file_index must be in [0, 256): read numbers are (file << 32 | read) in a 40-bit field");
    MatchCtx c;
    int rc = gs_db_get_info(db, &c.info);
    if (rc) return rc;
    const gs_host_match_opts none{};
    c.opts = &none;
    c.run = run;
    const double t_start = now_s();
    std::vector<int64_t> rof;
    bool composite = false;
    TrackerScope progress(paths, n_paths);
    const int err = run_files(c, paths, n_paths, file_index, rof, &composite);
    for (int i = 0; i < n_paths && (size_t)i < rof.size(); i++) reads_of_file[i] = rof[(size_t)i];
    if (totals) {
        totals->reads = c.reads;
        totals->kmers = c.kmers;
        totals->bps = c.bps;
        totals->filtered_reads = 0;
        totals->seconds_total = now_s() - t_start;
        totals->seconds_parse = c.t_parse;
        totals->seconds_gpu = c.t_gpu;
    }
    return err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

namespace {

struct FilterCtx {
    gs_bloom *bloom = nullptr;
    // the extract goal (gs_host_extract_files): no filter -- nextEntry is ByteArrayUtil.startsWith(readDescriptor, 1, key)
    // (C/goals/ExtractGoal.java:93), the same text stage on a gs_reads handle, everything else as the filter goal
    gs_reads *rd = nullptr;  // (reads: the counter below)
    std::string key;
    int k = 31, min_pos_count = 1;
    double positive_ratio = 0.2;
    bool with_probs = false;
    bool extract() const { return bloom == nullptr; }
    int get_device(int *device) { return extract() ? gs_reads_get_device(rd, device) : gs_filter_get_device(bloom, device); }
    int text_reset() { return extract() ? gs_reads_text_reset(rd, 1) : gs_filter_text_reset(bloom, 1); }
    int text_status(int64_t *failed, int64_t *bad, int64_t tot[3]) {
        return extract() ? gs_reads_text_status(rd, failed, bad, tot) : gs_filter_text_status(bloom, failed, bad, tot);
    }
    const uint8_t *key_bytes() const { return reinterpret_cast<const uint8_t *>(key.data()); }
    int submit_text(const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, uint8_t *acc, uint32_t *nl, int profile, int64_t *ticket) {
        if (extract()) return gs_reads_select_text(rd, k, text, n_bytes, n_lines, mem, key_bytes(), (int32_t)key.size(), acc, nl, ticket);
        return gs_filter_submit_text(bloom, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, mem, acc, nl, profile, ticket);
    }
    int submit_fasta(const uint8_t *text, int64_t n_bytes, int64_t n_lines, int64_t n_records, int mem, uint8_t *acc, uint32_t *nl, int64_t *ticket) {
        if (extract()) return gs_reads_select_fasta(rd, k, text, n_bytes, n_lines, n_records, mem, key_bytes(), (int32_t)key.size(), acc, nl, ticket);
        return gs_filter_submit_fasta(bloom, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, n_records, mem, acc, nl, ticket);
    }
    int submit_fastq_ml(const uint8_t *text, int64_t n_bytes, int64_t n_lines, int mem, uint8_t *acc, uint32_t *nl, int64_t *n_records, int64_t *used,
                        int64_t *lines, int64_t *ticket) {
        if (extract())
            return gs_reads_select_fastq_ml(rd, k, text, n_bytes, n_lines, mem, key_bytes(), (int32_t)key.size(), acc, nl, n_records, used, lines, ticket);
        return gs_filter_submit_fastq_ml(bloom, k, min_pos_count, positive_ratio, text, n_bytes, n_lines, mem, acc, nl, n_records, used, lines, ticket);
    }
    // records: the last chunk was FASTA or general FASTQ
    int compact_text(int which, int probs, int slot, const uint8_t **d_out, int64_t *n_bytes, int64_t *n_records, bool records = false) {
        if (records) {
            if (extract()) return gs_reads_compact_records(rd, probs, slot, d_out, n_bytes, n_records);
            return gs_filter_compact_records(bloom, which, probs, slot, d_out, n_bytes, n_records);
        }
        if (extract()) return gs_reads_compact_text(rd, probs, slot, d_out, n_bytes, n_records);  // (no rest file: which == 1)
        return gs_filter_compact_text(bloom, which, probs, slot, d_out, n_bytes, n_records);
    }
    int read_bounds(uint64_t *bounds) { return extract() ? gs_reads_text_read_bounds(rd, bounds) : gs_filter_text_read_bounds(bloom, bounds); }
    int line_classes(uint8_t *cls) { return extract() ? gs_reads_text_line_classes(rd, cls) : gs_filter_text_line_classes(bloom, cls); }
    // a parsed batch: the filter kernel, or the key against the descriptors where they lie
    int submit_batch(Batch &b, int64_t n) {
        if (!extract()) return gs_filter_submit(bloom, k, min_pos_count, positive_ratio, b.seq.data(), b.seq_off.data(), n, GS_MEM_HOST, accept.data(), 0);
        for (int64_t i = 0; i < n; i++) {
            const uint64_t d0 = b.desc_off[(size_t)i], d1 = b.desc_off[(size_t)i + 1];
            accept[(size_t)i] = d1 - d0 >= key.size() + 1 && memcmp(b.desc.data() + d0 + 1, key.data(), key.size()) == 0;
        }
        return GS_OK;
    }
    OutFile acc_out, rest_out;
    std::vector<uint8_t> accept;
    int64_t accepted = 0, reads = 0, kmers = 0, bps = 0;
    // progress records: the file being read and `reads` when it began; tot0 = reads of the file's accepted text chunks so far
    int prog_file = 0;
    int64_t prog_reads0 = 0;
    int64_t file_reads(int64_t tot0) const { return reads - prog_reads0 + tot0; }
    // a stop on request, when nothing of the file is in flight any more: the chunks the device took are counted, the record goes out
    void stop_record(const int64_t tot[3]) {
        reads += tot[0];
        kmers += tot[1];
        bps += tot[2];
        trk().stopped(prog_file, reads - prog_reads0);
    }
    double t_gpu = 0, t_parse = 0;
    FormatPool pool{format_threads()};
    DeviceWriter acc_dev, rest_dev;  // (declared behind the files: they wait for their writes before the files close)
};

struct FilterPart {
    std::vector<uint8_t> acc, rest;
    bool acc_packed = false, rest_packed = false;
    int64_t n_accepted = 0;
    void pack(OutFile &a, OutFile &r) {
        const size_t worth_it = (size_t)64 << 10;
        acc_packed = a.gzip() && acc.size() >= worth_it && a.pack(acc);
        rest_packed = r.gzip() && rest.size() >= worth_it && r.pack(rest);
    }
};

void write_filter_parts(FilterCtx &c, std::vector<FilterPart> &parts) {
    for (FilterPart &p : parts) {
        c.accepted += p.n_accepted;
        c.acc_out.write(std::move(p.acc), p.acc_packed);
        c.rest_out.write(std::move(p.rest), p.rest_packed);
    }
}

// reads per batch of the reference-exact parser in the filter / extract goal (GS_HOST_BATCH_READS; the match goal: batch_reads)
inline int64_t parser_batch_reads() {
    if (const char *e = getenv("GS_HOST_BATCH_READS")) {
        const long long v = atoll(e);
        if (v >= 1) return (int64_t)v;
    }
    return (int64_t)1 << 20;
}

// the general path for one source (file from `offset`, or a memory range): reference parser -> batches -> GPU -> writers
int filter_parsed_source(FilterCtx &c, const std::string &path, int64_t offset, const uint8_t *mem, size_t mem_n, bool mem_fasta = false) {
    Producer prod;
    prod.start(path, offset, mem, mem_n, c.k, parser_batch_reads(), mem_fasta);
    int err = GS_OK;
    Tracker &tk = trk();
    int64_t seen[3] = {0, 0, 0};  // reads, k-mers, bases of the batches that went through (what counts after a stop)
    bool stopped = false;
    for (;;) {
        std::unique_ptr<Batch> b = prod.q.pop();
        if (!b) break;
        if (err) continue;
        const int64_t n = b->n();
        c.accept.resize((size_t)n);
        if (b->seq.empty()) b->seq.push_back(0);
        const double t0 = now_s();
        err = c.submit_batch(*b, n);
        c.t_gpu += now_s() - t0;
        if (err) continue;
        std::vector<FilterPart> parts((size_t)c.pool.threads());
        const Batch &bb = *b;
        c.pool.run(n, [&](int t, int64_t lo, int64_t hi) {
            FilterPart &p = parts[(size_t)t];
            p.acc = c.acc_out.take();
            p.rest = c.rest_out.take();
            for (int64_t i = lo; i < hi; i++) {  // nextEntry (FastqBloomFilter.java:92-105), input order
                if (c.accept[(size_t)i]) {
                    p.n_accepted++;
                    if (c.acc_out.active()) append_read(p.acc, bb, i, c.with_probs);
                } else if (c.rest_out.active())
                    append_read(p.rest, bb, i, c.with_probs);
            }
            p.pack(c.acc_out, c.rest_out);
        });
        write_filter_parts(c, parts);
        if (tk.on()) {
            for (int64_t i = 0; i < n; i++) {
                const int64_t L = (int64_t)(bb.seq_off[(size_t)i + 1] - bb.seq_off[(size_t)i]);
                seen[1] += L >= c.k ? L - c.k + 1 : 0;
                seen[2] += L;
            }
            seen[0] += n;
            if (tk.chunk(c.prog_file, path.empty() ? 0 : bb.src_pos, false, c.file_reads(seen[0]))) {
                prod.stop.store(true);  // (what it has parsed beyond this batch is dropped, above)
                stopped = true;
                err = GS_E_CANCELLED;
            }
        }
    }
    prod.th.join();
    if (stopped) {
        c.t_parse += prod.seconds;
        c.stop_record(seen);
        return cancelled_rc();
    }
    if (!err && !prod.error.empty()) err = hfail(GS_E_INVALID, prod.error);
    c.reads += prod.reads;
    c.kmers += prod.kmers;
    c.bps += prod.bps;
    c.t_parse += prod.seconds;
    return err;
}

int filter_general_file(FilterCtx &c, const std::string &path, bool gzip, bool fasta);
int filter_files(FilterCtx &c, const char *const *paths, int n_paths, int extract_device, gs_host_totals *totals);

// the records of one chunk of four-line FASTQ to the writers: nextEntry (FastqBloomFilter.java:92-105), input order
void format_text_chunk(FilterCtx &c, const uint8_t *start, const uint8_t *h_acc, const uint32_t *h_nl, int64_t n_reads) {
    std::vector<FilterPart> parts((size_t)c.pool.threads());
    c.pool.run(n_reads, [&](int t, int64_t lo, int64_t hi) {
        FilterPart &p = parts[(size_t)t];
        p.acc = c.acc_out.take();
        p.rest = c.rest_out.take();
        for (int64_t r = lo; r < hi; r++) {
            if (h_acc[r]) {
                p.n_accepted++;
                if (c.acc_out.active()) append_text_record(p.acc, start, h_nl, r, c.with_probs);
            } else if (c.rest_out.active())
                append_text_record(p.rest, start, h_nl, r, c.with_probs);
        }
        p.pack(c.acc_out, c.rest_out);
    });
    write_filter_parts(c, parts);
}

// The back half of a four-line chunk of the filter / extract goal whose accept flags are in, device output: the writers' side stays
// on the device -- the records each file wants are gathered there (gs_filter_compact_text), a .gz file's are compressed there
// (DeviceWriter::emit -> gs_deflater_pack), and only what the files will hold crosses PCIe, on a thread of its own (dev_job) while
// the next chunk is read or inflated and filtered.  The chunk's text is on the device already: its block may go back at once.
// records: a FASTA or general FASTQ chunk (gs_filter_compact_records / gs_reads_compact_records), the same way out.
int filter_emit_device(FilterCtx &c, int set, int64_t n_reads, const uint8_t *h_acc, std::future<int> &dev_job, bool records = false) {
    static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
    const double t0 = now_s();
    const uint8_t *d_a = nullptr, *d_r = nullptr;
    int64_t nb_a = 0, nr_a = 0, nb_r = 0, nr_r = 0;
    int err = GS_OK;
    if (c.acc_out.active()) err = c.compact_text(1, c.with_probs ? 1 : 0, set, &d_a, &nb_a, &nr_a, records);
    if (!err && c.rest_out.active()) err = c.compact_text(0, c.with_probs ? 1 : 0, set, &d_r, &nb_r, &nr_r, records);
    if (err) return err;
    if (c.acc_out.active())
        c.accepted += nr_a;
    else if (c.rest_out.active())
        c.accepted += n_reads - nr_r;
    else
        for (int64_t r = 0; r < n_reads; r++) c.accepted += h_acc[r] != 0;
    const double t1 = now_s();
    if (dev_job.valid() && (err = dev_job.get())) return err;  // one chunk at a time: output order
    if (trace)
        fprintf(stderr, "filter chunk (device output): gather %.2f ms (%lld + %lld bytes), writers of the chunk before %.2f\n", (t1 - t0) * 1e3, (long long)nb_a, (long long)nb_r,
                (now_s() - t1) * 1e3);
    run_behind(dev_job, [&c, set, d_a, nb_a, d_r, nb_r]() -> int {
        const int e1 = c.acc_dev.emit(set, d_a, nb_a);
        const int e2 = c.rest_dev.emit(set, d_r, nb_r);
        return e1 ? e1 : e2;
    });
    return GS_OK;
}

// ... host output: the chunk's text, accept flags and newline offsets are on the host; the records are formatted and handed to the
// writers on a thread of their own (`formatting`), which ends with release() -- what gives the text's block back, if anything
void filter_emit_host(FilterCtx &c, const uint8_t *text, const uint8_t *h_acc, const uint32_t *h_nl, int64_t n_reads, std::future<void> &formatting,
                      std::function<void()> release) {
    static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
    const double t0 = now_s();
    if (formatting.valid()) formatting.get();  // one chunk at a time: output order, the other result set is free
    if (trace) fprintf(stderr, "filter chunk (host output): writers of the chunk before %.2f ms\n", (now_s() - t0) * 1e3);
    run_behind(formatting, [&c, text, h_acc, h_nl, n_reads, release] {
        format_text_chunk(c, text, h_acc, h_nl, n_reads);
        if (release) release();
    });
}

// The end of a file of the filter / extract goal whose text pipeline stopped without an error: the totals of the chunks the device
// took, then the rest -- from fallback_off on (>= 0: a chunk was refused, or cannot be cut) or what the last chunk left over.
// general_allowed: a FASTQ file that is not four lines per record from its very first chunk goes once more with the records found
// on the device (GS_HOST_ML=0: straight to the reference-exact parser, which also takes over whatever that pass refuses).
int filter_file_end(FilterCtx &c, const std::string &path, bool gzip, const int64_t tot[3], int64_t fallback_off, const std::vector<uint8_t> &carry, bool general_allowed,
                    bool fasta) {
    c.reads += tot[0];
    c.kmers += tot[1];
    c.bps += tot[2];
    if (fallback_off >= 0) {
        const int err = c.text_reset();
        if (err) return err;
        bool ml = general_allowed && fallback_off == 0;
        if (const char *e = getenv("GS_HOST_ML")) ml = ml && atoi(e) != 0;
        if (ml) return filter_general_file(c, path, gzip, false);
        return filter_parsed_source(c, path, fallback_off, nullptr, 0);
    }
    if (!carry.empty()) return filter_parsed_source(c, std::string(), 0, carry.data(), carry.size(), fasta);
    return GS_OK;
}

// Gzip FASTQ inflated on the device (DeviceInflate: block-gzip by its members, any other stream as a whole): the COMPRESSED bytes go
// to the device, the filter runs on the text where it lies (GS_MEM_DEVICE_TEXT), and the text comes back ONCE, page-locked, for the
// writers -- while the filter kernel runs -- or not at all (device output).  *handled = false: the caller takes its usual path.
int filter_bgzf_file(FilterCtx &c, const std::string &path, bool *handled) {
    *handled = false;
    size_t block;
    int readers = 0, device = 0;
    reader_shape(true, &block, &readers);
    TextReader tr;  // (for the mapping only: its readers are never started)
    DeviceInflate dev;
    if (tr.open(path, block, readers, true) == GS_OK && c.get_device(&device) == GS_OK) dev.open(tr.map, tr.map_len, device, gunzip_first_span());
    if (!dev.bgzf() && !dev.whole()) {
        tr.close();
        return GS_OK;
    }
    *handled = true;
    int err = c.text_reset();
    PooledBuf text_sets[2], nl_sets[2];
    PinnedVec<uint8_t> acc_sets[2];
    std::future<void> formatting;
    std::future<int> dev_job;  // device output: gather -> (deflate) -> fetch -> writer of the chunk before
    c.acc_dev.begin(&c.acc_out, device);
    c.rest_dev.begin(&c.rest_out, device);
    int64_t n_formatted = 0, text_off = 0, fallback_off = -1;
    int64_t tot[3] = {0, 0, 0}, failed = -1, bad = -1;
    bool stopped = false;  // a stop on request: the record goes out when the writers are through, before the decoder is handed back
    std::vector<uint8_t> carry;
    const double t0 = now_s();
    // (feeds of 128 MiB here, not 512: the writers get their first chunk four times earlier, and what they have not written when
    // the last feed is through is what the file waits for in the end -- 4 M reads: 285 ms with 512 MiB feeds, 175 ms with 128)
    // (with the writers' side on the device -- nothing to format, a sixth of the bytes to write -- the feeds are 256 MiB: 12.1 against
    // 11.2 Gbp/s gz -> gz at 16 M reads)
    const bool dev_out = device_output();
    const int64_t text_target = getenv("GS_HOST_BGZF_TEXT") ? bgzf_text_target() : ((int64_t)(dev_out ? 256 : 128) << 20);
    static const bool trace = getenv("GS_HOST_TRACE") != nullptr;
    while (!err) {
        DevText t;
        bool refused = false;
        const double tg = now_s();
        // (whole stream: every earlier slice has been waited for, gs_filter_text_status -- nothing reads the text a new batch replaces)
        err = dev.whole() ? dev.slices.next(text_target, path, nullptr, &t, &refused) : dev.feeds.next(text_target, path, &t);
        if (err) break;
        if (refused || t.stuck) {  // the host decoders / the general parser from here
            fallback_off = text_off;
            break;
        }
        if (t.n_lines > 0) {
            const int64_t n_reads = t.n_lines >> 2;
            const int set = (int)(n_formatted & 1);  // (the set of the chunk before last: its writers are through)
            if ((err = acc_sets[set].resize((size_t)n_reads))) break;
            if (!dev_out && ((err = nl_sets[set].need(sizeof(uint32_t) * (size_t)t.n_lines)) || (err = text_sets[set].need((size_t)t.n_bytes)))) break;
            uint8_t *h_acc = acc_sets[set].data(), *h_text = static_cast<uint8_t *>(text_sets[set].p);
            uint32_t *h_nl = static_cast<uint32_t *>(nl_sets[set].p);
            int64_t ticket = -1;
            const double t1 = now_s();
            err = c.submit_text(t.text, t.n_bytes, t.n_lines, GS_MEM_DEVICE_TEXT, h_acc, dev_out ? nullptr : h_nl, 0, &ticket);
            const double t2 = now_s();
            if (!err && !dev_out) err = dev.whole() ? dev.slices.fetch_text(t, h_text) : dev.feeds.fetch_text(h_text, t.n_bytes);  // (while the kernel runs)
            const double t3 = now_s();
            if (!err) err = c.text_status(&failed, &bad, tot);  // synchronises: results are needed now
            const double t4 = now_s();
            c.t_gpu += t4 - tg;
            if (err) break;
            if (failed >= 0) {  // not four-line FASTQ from here on: the general parser continues at this chunk
                fallback_off = text_off;
                break;
            }
            if (trace)
                fprintf(stderr, "filter feed: %lld bytes, inflate + buffers %.2f ms, submit %.2f, text back %.2f, status %.2f\n", (long long)t.n_bytes, (t1 - tg) * 1e3,
                        (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3);
            if (dev_out) {
                if ((err = filter_emit_device(c, set, n_reads, h_acc, dev_job))) break;
            } else
                filter_emit_host(c, h_text, h_acc, h_nl, n_reads, formatting, nullptr);
            n_formatted++;
            text_off += t.n_bytes;
            const bool members = dev.bgzf() && dev.feeds.next_member < dev.feeds.members.size();  // (they say where they lie in the file)
            if (trk().chunk(c.prog_file, members ? dev.feeds.members[dev.feeds.next_member].payload_offset : text_off, !members, c.file_reads(tot[0]))) {
                stopped = true;
                break;
            }
        }
        if (t.last) {  // what is left behind the last whole record
            err = dev.whole() ? dev.slices.fetch_leftover(carry) : dev.feeds.fetch_tail(carry);
            break;
        }
    }
    const double te0 = now_s();
    if (formatting.valid()) formatting.get();
    if (dev_job.valid()) {
        const int e2 = dev_job.get();
        if (!err) err = e2;
    }
    const double te1 = now_s();
    if (stopped && !err) c.stop_record(tot);
    dev.close();  // (every slice's filter run has been waited for: gs_filter_text_status)
    tr.close();
    if (trace)
        fprintf(stderr, "filter bgzf: loop %.2f ms (from open), last writers %.2f, inflater back + unmap %.2f\n", (te0 - t0) * 1e3, (te1 - te0) * 1e3, (now_s() - te1) * 1e3);
    c.t_parse += now_s() - t0;
    if (err) return err;
    if (stopped) return cancelled_rc();
    return filter_file_end(c, path, true, tot, fallback_off, carry, true, false);
}

// plain FASTQ: raw text blocks to the device (gs_filter_submit_text); accept flags and record geometry come back
int filter_text_file(FilterCtx &c, const std::string &path, bool gzip) {
    size_t block;
    int readers = 0;
    reader_shape(gzip, &block, &readers);
    TextReader tr;
    int err = tr.open(path, block, readers, gzip);
    if (err) {
        tr.close();
        return err;
    }
    err = c.text_reset();
    // results of a chunk land in pinned memory: accept flags + newline offsets; two sets, so that the writers can work
    // on one chunk (on a thread of their own) while the device is busy with the next
    PinnedVec<uint8_t> acc_sets[2];
    PinnedVec<uint32_t> nl_sets[2];
    std::future<void> formatting;
    std::future<int> dev_job;
    // (plain outputs from a plain file are formatted from the reader's page-locked block, which is on the host anyway)
    int device = 0;
    const bool dev_out = device_output() && ((c.acc_out.active() && c.acc_out.gzip()) || (c.rest_out.active() && c.rest_out.gzip())) &&
                         c.get_device(&device) == GS_OK;
    c.acc_dev.begin(&c.acc_out, device);
    c.rest_dev.begin(&c.rest_out, device);
    int64_t n_formatted = 0, fallback_off = -1;
    ChunkCutter cut;
    int64_t tot[3] = {0, 0, 0}, failed = -1, bad = -1;
    bool stopped = false;  // a stop on request: the record goes out when the writers are through, before the readers are stopped
    const double t0 = now_s();
    if (!err) tr.start();
    for (int64_t i = 0; !err; i++) {
        TextSlot &sl = tr.wait_full(i);
        if ((err = block_error(tr, sl, path))) break;
        const bool eof = sl.eof;
        bool keep_block = false;
        const ChunkCutter::Cut what = cut_block(cut, tr, sl);
        if (what == ChunkCutter::FALLBACK) {
            fallback_off = cut.file_off;
        } else if (what == ChunkCutter::CHUNK) {
            const int64_t n_reads = cut.lines >> 2;
            const int set = (int)(n_formatted & 1);  // (the set of the chunk before last)
            if ((err = acc_sets[set].resize((size_t)n_reads))) break;
            if ((err = nl_sets[set].resize((size_t)cut.lines))) break;
            uint8_t *h_acc = acc_sets[set].data();
            uint32_t *h_nl = nl_sets[set].data();
            int64_t ticket = -1;
            const double tg = now_s();
            err = c.submit_text(cut.start, cut.bytes, cut.lines, GS_MEM_HOST, h_acc, h_nl, 0, &ticket);
            if (!err) err = c.text_status(&failed, &bad, tot);  // synchronises: results are needed now
            c.t_gpu += now_s() - tg;
            if (err) break;
            if (failed >= 0) {  // not four-line FASTQ from here on: the general parser continues at this chunk
                fallback_off = cut.file_off;
            } else {
                const uint8_t *start = cut.start;
                cut.commit();  // (the carry is taken out first: the block returns to its reader when the writers are through with it)
                if (dev_out) {  // a .gz output: the block goes straight back to its reader
                    if ((err = filter_emit_device(c, set, n_reads, h_acc, dev_job))) break;
                } else {
                    keep_block = true;
                    filter_emit_host(c, start, h_acc, h_nl, n_reads, formatting, [&tr, i] { tr.release(i); });
                }
                n_formatted++;
                stopped = trk().chunk(c.prog_file, cut.file_off, gzip, c.file_reads(tot[0]));
                if (stopped) break;  // (a block that nobody formats from stays where it is until the readers are stopped)
            }
        }
        if (!keep_block) tr.release(i);
        if (eof || fallback_off >= 0) break;
    }
    if (formatting.valid()) formatting.get();
    if (dev_job.valid()) {
        const int e2 = dev_job.get();
        if (!err) err = e2;
    }
    if (stopped && !err) c.stop_record(tot);
    tr.close();
    c.t_parse += now_s() - t0;
    if (err) return err;
    if (stopped) return cancelled_rc();
    return filter_file_end(c, path, gzip, tot, fallback_off, cut.carry, true, false);
}

// FASTA and general FASTQ (sequence / quality over several lines): chunks of whole records (FASTA: cut in front of a header
// line) or of whole lines (general FASTQ: the device says how many records end in the chunk and what they cover) go to the
// device (gs_filter_submit_fasta / gs_filter_submit_fastq_ml); every record is written as four-line FASTQ.  What the device
// refuses and the tail of the file go through the reference-exact parser.
int filter_general_file(FilterCtx &c, const std::string &path, bool gzip, bool fasta) {
    size_t block;
    int readers = 0;
    reader_shape(gzip, &block, &readers);
    TextReader tr;
    int err = tr.open(path, block, readers, gzip);
    if (err) {
        tr.close();
        return err;
    }
    err = c.text_reset();
    // two result sets: the records of chunk i are formatted and handed to the writers on a thread of their own while chunk i + 1 is
    // on the device (as the four-line path does; the chunk's block goes back to its reader when the formatting is through)
    struct Res {
        PinnedVec<uint8_t> acc;
        PinnedVec<uint32_t> nls;
        std::vector<uint64_t> bounds;
        std::vector<uint8_t> cls;
        std::vector<int64_t> head;
    } res[2];
    std::future<void> formatting;
    // device output under the condition of the four-line chunks of filter_text_file (GS_DEVICE_RECORDS=0: the host's formatter): the
    // records each file wants are written on the device, the chunk's block goes straight back to its reader
    std::future<int> dev_job;
    int device = 0;
    const bool dev_out = device_records() && device_output() &&
                         ((c.acc_out.active() && c.acc_out.gzip()) || (c.rest_out.active() && c.rest_out.gzip())) && c.get_device(&device) == GS_OK;
    c.acc_dev.begin(&c.acc_out, device);
    c.rest_dev.begin(&c.rest_out, device);
    int64_t n_chunks = 0, fallback_off = -1;
    ChunkCutter cut;
    cut.mode = fasta ? ChunkCutter::FASTA : ChunkCutter::GENERAL;
    int64_t tot[3] = {0, 0, 0}, failed = -1, bad = -1;
    bool stopped = false;  // a stop on request: the record goes out when the writers are through, before the readers are stopped
    const double t0 = now_s();
    if (!err) tr.start();
    for (int64_t i = 0; !err; i++) {
        TextSlot &sl = tr.wait_full(i);
        if ((err = block_error(tr, sl, path))) break;
        const bool eof = sl.eof;
        const ChunkCutter::Cut what = cut_block(cut, tr, sl);
        if (what == ChunkCutter::FALLBACK) {  // a record longer than a block, more records than one chunk may hold
            fallback_off = cut.file_off;
        } else if (what == ChunkCutter::CHUNK) {
            const uint8_t *start = cut.start;
            Res &rs = res[n_chunks & 1];
            PinnedVec<uint8_t> &acc = rs.acc;
            PinnedVec<uint32_t> &nls = rs.nls;
            std::vector<uint64_t> &bounds = rs.bounds;
            std::vector<uint8_t> &cls = rs.cls;
            std::vector<int64_t> &head = rs.head;
            std::function<void()> format_job;
            const int64_t bytes = cut.bytes;
            int64_t lines = cut.lines, records = cut.records, used = bytes, ticket = -1;
            if (bytes > 0) {
                if ((err = acc.resize((size_t)(fasta ? std::max<int64_t>(records, 1) : lines / 4 + 2)))) break;
                if ((err = nls.resize((size_t)std::max<int64_t>(lines, 1)))) break;
                const double tg = now_s();
                if (fasta)
                    err = c.submit_fasta(start, bytes, lines, records, GS_MEM_HOST, acc.data(), nls.data(), &ticket);
                else  // (the device says what its records cover: `used` bytes, `lines` lines)
                    err = c.submit_fastq_ml(start, bytes, cut.lines, GS_MEM_HOST, acc.data(), nls.data(), &records, &used, &lines, &ticket);
                if (!err) err = c.text_status(&failed, &bad, tot);  // synchronises: results are needed now
                if (!err && failed < 0 && records > 0 && !dev_out) {
                    bounds.resize((size_t)records + 1);
                    cls.resize((size_t)lines);
                    err = c.read_bounds(bounds.data());
                    if (!err && !fasta) err = c.line_classes(cls.data());
                }
                c.t_gpu += now_s() - tg;
                if (err) break;
                if (failed >= 0 || records < 0) {  // refused: the general parser continues at this chunk
                    fallback_off = cut.file_off;
                } else if (records > 0 && dev_out) {
                    g_filter_general_chunks.fetch_add(1);
                    if ((err = filter_emit_device(c, (int)(n_chunks & 1), records, acc.data(), dev_job, true))) break;
                    g_record_device_chunks.fetch_add(1);
                    n_chunks++;
                } else if (records > 0) {
                    g_filter_general_chunks.fetch_add(1);
                    const uint32_t *nl = nls.p;
                    auto line_start = [nl](int64_t j) { return j ? (size_t)nl[j - 1] + 1 : (size_t)0; };
                    if (fasta)
                        for (int64_t j = 0; j < lines; j++) cls[(size_t)j] = start[line_start(j)] == '>' && nl[j] > line_start(j) ? 1 : 2;
                    head.clear();  // descriptor line of every record, + lines
                    for (int64_t j = 0; j < lines; j++)
                        if (cls[(size_t)j] == 1) head.push_back(j);
                    if ((int64_t)head.size() != records) {
                        err = hfail(GS_E_INVALID, "text chunk: the descriptor lines do not match the device's record count");
                        break;
                    }
                    head.push_back(lines);
                    const bool probs = c.with_probs && !fasta;
                    const int64_t n_rec = records;
                    Res *rp = &rs;
                    format_job = [&c, rp, start, nl, n_rec, fasta, probs] {
                        std::vector<FilterPart> parts((size_t)c.pool.threads());
                        const Res &r_ = *rp;
                        c.pool.run(n_rec, [&](int t, int64_t lo, int64_t hi) {
                            FilterPart &p = parts[(size_t)t];
                            p.acc = c.acc_out.take();
                            p.rest = c.rest_out.take();
                            for (int64_t r = lo; r < hi; r++) {  // nextEntry (FastqBloomFilter.java:92-105), input order
                                const int64_t L = (int64_t)(r_.bounds[(size_t)r + 1] - r_.bounds[(size_t)r]);
                                if (r_.acc[(size_t)r]) {
                                    p.n_accepted++;
                                    if (c.acc_out.active())
                                        append_general_record(p.acc, start, nl, r_.cls.data(), r_.head[(size_t)r], r_.head[(size_t)r + 1], L, fasta, probs);
                                } else if (c.rest_out.active())
                                    append_general_record(p.rest, start, nl, r_.cls.data(), r_.head[(size_t)r], r_.head[(size_t)r + 1], L, fasta, probs);
                            }
                            p.pack(c.acc_out, c.rest_out);
                        });
                        write_filter_parts(c, parts);
                    };
                }
            }
            if (fallback_off < 0) cut.commit(used, lines);  // (general FASTQ: what the records did not cover is carried as well)
            if (format_job) {  // (the carry has been taken out of the block: the formatting thread may hand it back)
                if (formatting.valid()) formatting.get();  // one chunk at a time: output order, and the other result set is free again
                n_chunks++;
                run_behind(formatting, [format_job, &tr, i] {
                    format_job();
                    tr.release(i);
                });
                stopped = trk().chunk(c.prog_file, cut.file_off, gzip, c.file_reads(tot[0]));
                if (eof || fallback_off >= 0 || stopped) break;
                continue;
            }
            stopped = fallback_off < 0 && trk().chunk(c.prog_file, cut.file_off, gzip, c.file_reads(tot[0]));
            if (stopped) break;  // (the block stays where it is until the readers are stopped)
        }
        tr.release(i);
        if (eof || fallback_off >= 0) break;
    }
    if (formatting.valid()) formatting.get();
    if (dev_job.valid()) {
        const int e2 = dev_job.get();
        if (!err) err = e2;
    }
    if (stopped && !err) c.stop_record(tot);
    tr.close();
    c.t_parse += now_s() - t0;
    if (err) return err;
    if (stopped) return cancelled_rc();
    return filter_file_end(c, path, gzip, tot, fallback_off, cut.carry, false, fasta);
}

}  // namespace

extern "C" int gs_host_filter_files(gs_bloom *bloom, int k, int min_pos_count, double positive_ratio,
                                    const char *const *paths, int n_paths, const char *filtered_path,
                                    const char *rest_path, int with_probs, gs_host_totals *totals) try {
    if (!bloom || !paths || n_paths < 0) return hfail(GS_E_INVALID, "NULL argument");
    FilterCtx c;
    c.with_probs = with_probs != 0;
    c.bloom = bloom;
    c.k = k;
    c.min_pos_count = min_pos_count;
    c.positive_ratio = positive_ratio;
    if (!c.acc_out.open(filtered_path) || !c.rest_out.open(rest_path)) return hfail(GS_E_INVALID, "cannot open output file");
    return filter_files(c, paths, n_paths, -1, totals);
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

namespace {
// the files in order through the text pipelines (GS_HOST_FAST=0: all of them through the reference-exact parser); extract_device
// >= 0: the extract goal, whose gs_reads handle is made here when the first file needs it -- the parser's path needs no device
int filter_files(FilterCtx &c, const char *const *paths, int n_paths, int extract_device, gs_host_totals *totals) {
    const double t_start = now_s();
    const bool trace = getenv("GS_HOST_TRACE") != nullptr;
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    int err = GS_OK;
    TrackerScope progress(paths, n_paths);
    Tracker &tk = progress.t;
    for (int f = 0; f < n_paths && !err; f++) {
        c.prog_file = f;
        c.prog_reads0 = c.reads;
        if (tk.file_start(f)) {
            tk.stopped(f, 0);
            err = cancelled_rc();
            break;
        }
        if (fast && extract_device >= 0 && !c.rd && gs_reads_create(&c.rd, extract_device) != GS_OK) {
            err = hfail(GS_E_HIP, gs_last_error());
            break;
        }
        if (trace && c.rd) gs_reads_kernel_time(c.rd, 1, nullptr, nullptr);  // (the handle's phases between events from here on)
        const std::string path(paths[f]);
        const int kind = fast ? text_path_kind(path) : 0;
        if (kind >= 3)
            err = filter_general_file(c, path, kind == 4, true);
        else if (kind) {
            bool handled = false;
            if (kind == 2) err = filter_bgzf_file(c, path, &handled);  // (block-gzip: inflated on the device)
            if (!err && !handled) err = filter_text_file(c, path, kind == 2);
        }
        else
            err = filter_parsed_source(c, path, 0, nullptr, 0);
        if (!err && tk.file_end(f, c.reads - c.prog_reads0)) err = cancelled_rc();
    }
    if (!err && tk.close()) err = cancelled_rc();
    const bool stopped = err == GS_E_CANCELLED;  // a stop on request: the outputs are closed as after a whole run, then the code
    if (stopped) err = GS_OK;
    const double tc0 = now_s();
    const bool wrote = c.acc_out.close() & c.rest_out.close();
    if (!err) err = c.acc_dev.late_err ? c.acc_dev.late_err : c.rest_dev.late_err;
    if (trace) fprintf(stderr, "filter files: %.2f ms before the outputs were closed, closing %.2f ms\n", (tc0 - t_start) * 1e3, (now_s() - tc0) * 1e3);
    if (trace && c.rd) {  // the extract goal, phase by phase
        int64_t n[3] = {0, 0, 0};
        double ms[3] = {0, 0, 0};
        if (gs_reads_phase_times(c.rd, n, ms) == GS_OK)
            fprintf(stderr,
                    "extract phases: files %.2f ms (device calls %.2f ms of them), closing the output %.2f ms; on the stream: select %lld chunks %.3f ms, "
                    "four-line gather %lld calls %.3f ms, FASTA text %lld calls %.3f ms\n",
                    (tc0 - t_start) * 1e3, c.t_gpu * 1e3, (now_s() - tc0) * 1e3, (long long)n[0], ms[0], (long long)n[1], ms[1], (long long)n[2], ms[2]);
    }
    if (!err && !wrote) err = hfail(GS_E_IO, "write to an output file failed");
    if (totals) {
        totals->reads = c.reads;
        totals->kmers = c.kmers;
        totals->bps = c.bps;
        totals->filtered_reads = c.accepted;
        totals->seconds_total = now_s() - t_start;
        totals->seconds_parse = c.t_parse;
        totals->seconds_gpu = c.t_gpu;
    }
    return !err && stopped ? cancelled_rc() : err;
}
}  // namespace

// The pools above keep page-locked blocks and the device decoders' buffers (a parked gunzipper holds up to a quarter of the free
// HBM) for the life of the process.  A long-lived host -- a JVM that next loads a big store -- hands them back with this call;
// nothing may be using the host layer on another thread meanwhile.
namespace {
void release_pools_impl() {
    {
        PinnedPool &pp = pinned_pool();  // (the big buffers of this file)
        std::lock_guard<std::mutex> l(pp.m);
        for (auto &x : pp.idle) gs_pinned_free(x.first);
        pp.idle.clear();
    }
    gs_host::pinned_pool().release_all();  // (the readers' blocks)
    {
        InflaterPool &ip = inflater_pool();
        std::lock_guard<std::mutex> l(ip.m);
        for (auto &x : ip.idle) gs_inflater_destroy(x.second);
        ip.idle.clear();
    }
    {
        GunzipperPool &gp = gunzipper_pool();
        std::lock_guard<std::mutex> l(gp.m);
        for (auto &x : gp.idle) gs_gunzipper_close(x.second);
        gp.idle.clear();
    }
    {
        DeflaterPool &dp = deflater_pool();
        std::lock_guard<std::mutex> l(dp.m);
        for (auto &x : dp.idle) gs_deflater_destroy(x.second);
        dp.idle.clear();
    }
}
}  // namespace

extern "C" int gs_host_release_pools(void) try {
    release_pools_impl();
    gs_device_cache_trim();  // (the pools' device memory went through the C ABI library's block cache)
    return GS_OK;
} catch (const std::exception &e) {  // (nothing may leave through the C ABI)
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

extern "C" int64_t gs_host_stat(int which) {
    switch (which) {
        case 0: return g_ml_chunks.load();
        case 5: return g_krakencount_chunks.load();
        case 1: return g_filter_general_chunks.load();
        case 2: return g_kraken_device_chunks.load();
        case 3: return g_record_device_chunks.load();
        default: return -1;
    }
}

// ---- db2fastq (C/goals/DB2FastqGoal.java -> KMerFastqGenerator.generateFastq): the text is made on the device chunk by chunk
// (gs_dbexport_fastq_next) and leaves it as the file's bytes, compressed there for a .gz name (DeviceWriter, as the per-read writers)
extern "C" int gs_host_db2fastq(gs_db *db, const char *const *taxids, const char *project, int32_t sel_vi, int with_desc, const char *path,
                                int64_t *n_written) try {
    if (!db || !taxids || !project || !path) return hfail(GS_E_INVALID, "NULL argument");
    gs_dbexport *x = nullptr;
    int64_t n = 0;
    if (gs_dbexport_create(&x, db, sel_vi, with_desc, &n) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
    std::unique_ptr<gs_dbexport, int (*)(gs_dbexport *)> hold(x, gs_dbexport_destroy);
    int device = 0;
    gs_dbexport_get_device(x, &device);
    if (gs_dbexport_fastq_begin(x, taxids, project) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
    OutFile out;
    if (!out.open(path)) return hfail(GS_E_IO, std::string("cannot open ") + path);
    int err = GS_OK;
    {
        DeviceWriter w;
        w.begin(&out, device);
        for (;;) {
            const uint8_t *d_text = nullptr;
            int64_t n_bytes = 0, n_records = 0;
            if (gs_dbexport_fastq_next(x, &d_text, &n_bytes, &n_records) != GS_OK) {
                err = hfail(GS_E_HIP, gs_last_error());
                break;
            }
            if (n_records == 0) break;
            if ((err = w.emit(0, d_text, n_bytes)) != GS_OK) break;
        }
        const int e = w.finish();
        if (!err) err = e;
    }
    if (!out.close() && !err) err = hfail(GS_E_IO, std::string("writing ") + path + " failed");
    if (err) return err;
    if (n_written) *n_written = n;
    return GS_OK;
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

namespace {
// the gs_reads handle of a goal's context goes on every way out of the call, an exception included; declared behind the context,
// so the handle is gone before the context's writers are
// a handle of the C ABI that a file-level call made: destroyed on every way out, unless the call has handed it on (h = nullptr)
template <class H, int (*destroy)(H *)>
struct HandleGuard {
    H *&h;
    ~HandleGuard() {
        if (h) destroy(h);
        h = nullptr;
    }
};
}  // namespace

// ---- extract (C/goals/ExtractGoal.java:73-129): every read whose descriptor starts with the key -> out_path, written as
// ReadEntry.write with the goal's withProbs = true; files, readers, inflaters and writers are the filter goal's (filter_files)
extern "C" int gs_host_extract_files(int device, const char *key, int k, const char *const *paths, int n_paths, const char *out_path,
                                     gs_host_totals *totals) try {
    if (!key || !paths || n_paths < 0 || !out_path) return hfail(GS_E_INVALID, "NULL argument");
    if (k < 1 || k > 31) return hfail(GS_E_INVALID, "k must be in [1,31]");
    FilterCtx c;
    HandleGuard<gs_reads, gs_reads_destroy> guard{c.rd};
    c.key = key;
    if (c.key.empty()) return hfail(GS_E_INVALID, "the key is empty");
    for (unsigned char ch : c.key)  // (Java compares byte != char: a byte >= 0x80 never matches)
        if (ch >= 0x80) return hfail(GS_E_INVALID, "the key holds a byte >= 0x80");
    c.k = k;
    c.with_probs = true;
    if (!c.acc_out.open(out_path)) return hfail(GS_E_IO, std::string("cannot open ") + out_path);
    return filter_files(c, paths, n_paths, device, totals);
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- fasta2fastq (C/goals/Fasta2FastqGoal.java:92-165)
namespace {

struct F2fCtx {
    gs_reads *reads = nullptr;
    int device = 0;
    OutFile out;
    int64_t records = 0;
    int prog_file = 0;           // progress records: the file being read, `records` when it began, `records` at the last record
    int64_t prog_records0 = 0, prog_mark = 0;
    double t_read = 0, t_dev = 0, t_emit = 0, t_cpu = 0;  // waiting for blocks (read, inflate); device calls; handing text to the writer; f2f_cpu
    DeviceWriter dev;  // (declared behind the file: it waits for its writes before the file closes)
};

// PrintStream.print((char) b) of a UTF-8 stream: a byte >= 0x80 is sign-extended to the char 0xFF80 .. 0xFFFF and leaves as three bytes
void f2f_print(std::vector<uint8_t> &o, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (p[i] < 0x80) {
            o.push_back(p[i]);
        } else {
            const unsigned ch = 0xFF00u | p[i];
            o.push_back(0xEF);
            o.push_back((uint8_t)(0x80 | ((ch >> 6) & 0x3F)));
            o.push_back((uint8_t)(0x80 | (ch & 0x3F)));
        }
    }
}

// The goal's loop, line by line: AbstractFastaReader.readFasta (C/fasta/AbstractFastaReader.java:97-130) with the FastqWriter of
// Fasta2FastqGoal.java:118-165 over BufferedLineReader.nextLine (LineReader: NUL bytes dropped, the '\n' part of the line).  The
// file from `offset` on, or a memory range.  Text in front of a first header is printed raw, without a record; a final header
// line without '\n' loses its last byte (size - 1), a final data line without '\n' keeps all of its bytes.
int f2f_cpu(F2fCtx &c, const std::string &path, int64_t offset, const uint8_t *mem, size_t mem_n) {
    const double t_begin = now_s();
    LineReader lr;
    if (path.empty())
        lr.open_mem(mem, mem_n);
    else if (!lr.open(path, offset))
        return hfail(GS_E_IO, "cannot open " + path);
    std::vector<uint8_t> line, o = c.out.take();
    bool first = true;
    int64_t data_size = 0;
    Tracker &tk = trk();
    const int64_t step = parser_batch_reads();  // records per progress record (GS_HOST_BATCH_READS)
    // between two records: what has been printed goes to the writer, a progress record goes out; true: stop
    // (the buffer goes to the writer where it would without a control -- when it is full, at the end of the source -- or when the
    // call stops: a .gz output is packed buffer by buffer, and a control that is not cancelled must not move a member boundary)
    auto report = [&](bool last) {
        c.prog_mark = c.records;
        if (last) c.out.write(std::move(o));
        if (!tk.chunk(c.prog_file, path.empty() ? 0 : lr.raw_pos(), false, c.records - c.prog_records0)) return false;
        if (!last) c.out.write(std::move(o));
        tk.stopped(c.prog_file, c.records - c.prog_records0);
        c.t_cpu += now_s() - t_begin;
        return true;
    };
    auto end_region = [&] {
        o.push_back('\n');
        o.push_back('+');
        o.push_back('\n');
        o.insert(o.end(), (size_t)data_size, (uint8_t)'~');
        o.push_back('\n');
    };
    for (;;) {
        line.clear();
        const size_t size = lr.next_line(line);
        if (size == 0) break;
        if (size >= 65534) return hfail(GS_E_INVALID, "buffer is too small for data line in fasta file " + path);  // (a target of 65 535 bytes, :104-106)
        if (line[0] == '>') {
            if (!first) end_region();
            if (tk.on() && !first && c.records - c.prog_mark >= step && report(false)) return cancelled_rc();
            first = false;
            data_size = 0;
            c.records++;
            o.push_back('@');
            f2f_print(o, line.data() + 1, size >= 2 ? size - 2 : 0);  // println(target, 1, size - 1)
            o.push_back('\n');
        } else {
            size_t end = size;
            while (end > 0 && (line[end - 1] == '\n' || line[end - 1] == '\r')) end--;
            f2f_print(o, line.data(), end);
            data_size += (int64_t)end;
        }
        if (o.size() >= ((size_t)4 << 20)) {
            c.out.write(std::move(o));
            o = c.out.take();
        }
    }
    if (!first) end_region();
    if (tk.on()) return report(true) ? cancelled_rc() : (c.t_cpu += now_s() - t_begin, (int)GS_OK);
    c.out.write(std::move(o));
    c.t_cpu += now_s() - t_begin;
    return GS_OK;
}

bool f2f_high_bytes(const uint8_t *p, size_t n) {
    uint8_t any = 0;
    for (size_t i = 0; i < n; i++) any |= p[i];
    return (any & 0x80) != 0;
}

// One file through the device: chunks of whole records, cut in front of a header line (fasta_cut), become FASTQ text there
// (gs_reads_fasta2fastq) and leave it as the output file's bytes (DeviceWriter).  What the device refuses -- text in front of a
// first header, a NUL byte --, a record that does not fit a block, bytes >= 0x80 (the reference widens them) and the tail of a
// file without a final newline go through f2f_cpu from the start of that chunk.
int f2f_device_file(F2fCtx &c, const std::string &path, bool gzip) {
    size_t block;
    int readers = 0;
    reader_shape(gzip, &block, &readers);
    TextReader tr;
    int err = tr.open(path, block, readers, gzip);
    if (err) {
        tr.close();
        return err;
    }
    if (gs_reads_text_reset(c.reads, 1) != GS_OK) err = hfail(GS_E_HIP, gs_last_error());
    ChunkCutter cut;
    cut.mode = ChunkCutter::FASTA;
    int64_t fallback_off = -1, n_chunks = 0;
    bool stopped = false;  // a stop on request: the record goes out before the readers are stopped
    if (!err) tr.start();
    for (int64_t i = 0; !err; i++) {
        const double tw = now_s();
        TextSlot &sl = tr.wait_full(i);
        c.t_read += now_s() - tw;
        if ((err = block_error(tr, sl, path))) break;
        const bool eof = sl.eof;
        // (bytes >= 0x80 are looked for before the cut: the line-by-line loop starts in front of the carry)
        const ChunkCutter::Cut what = f2f_high_bytes(sl.buf + tr.headroom, sl.n) ? ChunkCutter::FALLBACK : cut_block(cut, tr, sl);
        if (what == ChunkCutter::FALLBACK) {  // (also: a record longer than a block, more records than one chunk may hold)
            fallback_off = cut.file_off;
        } else if (what == ChunkCutter::CHUNK) {
            const uint8_t *start = cut.start;
            const int64_t bytes = cut.bytes, lines = cut.lines, records = cut.records;
            if (bytes > 0) {
                const uint8_t *d_text = nullptr;
                int64_t n_out = 0, long_lines = 0, failed = -1, bad = -1, tot[3] = {0, 0, 0};
                const double td = now_s();
                if (gs_reads_fasta2fastq(c.reads, start, bytes, lines, records, GS_MEM_HOST, (int)(n_chunks & 1), &d_text, &n_out, &long_lines, nullptr) != GS_OK ||
                    gs_reads_text_status(c.reads, &failed, &bad, tot) != GS_OK) {
                    err = hfail(GS_E_HIP, gs_last_error());
                    break;
                }
                c.t_dev += now_s() - td;
                if (failed >= 0) {
                    fallback_off = cut.file_off;
                } else if (long_lines > 0) {
                    err = hfail(GS_E_INVALID, "buffer is too small for data line in fasta file " + path);
                    break;
                } else {
                    const double te = now_s();
                    err = c.dev.emit((int)(n_chunks & 1), d_text, n_out);
                    c.t_emit += now_s() - te;
                    if (err) break;
                    n_chunks++;
                    c.records += records;
                }
            }
            if (fallback_off < 0) {
                cut.commit();
                c.prog_mark = c.records;
                stopped = trk().chunk(c.prog_file, cut.file_off, gzip, c.records - c.prog_records0);
                if (stopped) break;  // (every chunk's text has left the device for the writer: DeviceWriter::emit)
            }
        }
        tr.release(i);
        if (eof || fallback_off >= 0) break;
    }
    if (stopped && !err) trk().stopped(c.prog_file, c.records - c.prog_records0);
    tr.close();
    if (err) return err;
    if (stopped) return cancelled_rc();
    if (fallback_off >= 0) {
        if (gs_reads_text_reset(c.reads, 1) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        return f2f_cpu(c, path, fallback_off, nullptr, 0);
    }
    if (!cut.carry.empty()) return f2f_cpu(c, std::string(), 0, cut.carry.data(), cut.carry.size());
    return GS_OK;
}

}  // namespace

extern "C" int gs_host_fasta2fastq(int device, const char *const *paths, int n_paths, const char *out_path, int64_t *n_records) try {
    if (!paths || n_paths < 0 || !out_path) return hfail(GS_E_INVALID, "NULL argument");
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    int err = GS_OK;
    int64_t records = 0;
    bool wrote = true, stopped = false;
    TrackerScope progress(paths, n_paths);
    Tracker &tk = progress.t;
    {
        F2fCtx c;
        HandleGuard<gs_reads, gs_reads_destroy> guard{c.reads};
        c.device = device;
        if (!c.out.open(out_path)) return hfail(GS_E_IO, std::string("cannot open ") + out_path);
        if (fast && gs_reads_create(&c.reads, device) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        const bool trace = getenv("GS_HOST_TRACE") != nullptr;
        if (trace && c.reads) gs_reads_kernel_time(c.reads, 1, nullptr, nullptr);  // (the text kernels between events from here on)
        c.dev.begin(&c.out, device);
        const double t_start = now_s();
        for (int f = 0; f < n_paths && !err; f++) {  // (all resources into ONE file, Fasta2FastqGoal.java:96-102)
            const std::string path(paths[f]);
            c.prog_file = f;
            c.prog_records0 = c.prog_mark = c.records;
            if (tk.file_start(f)) {
                tk.stopped(f, 0);
                err = cancelled_rc();
                break;
            }
            const int kind = fast ? text_path_kind(path) : 0;
            err = kind ? f2f_device_file(c, path, kind == 2 || kind == 4) : f2f_cpu(c, path, 0, nullptr, 0);
            if (!err && tk.file_end(f, c.records - c.prog_records0)) err = cancelled_rc();
        }
        if (!err && tk.close()) err = cancelled_rc();
        stopped = err == GS_E_CANCELLED;  // a stop on request: the output is closed as after a whole run, then the code
        if (stopped) err = GS_OK;
        const double tc0 = now_s();
        const int e2 = c.dev.finish();
        if (!err) err = e2;
        wrote = c.out.close();
        if (trace) {  // the goal, phase by phase
            int64_t n[3] = {0, 0, 0};
            double ms[3] = {0, 0, 0};
            if (c.reads) gs_reads_phase_times(c.reads, n, ms);
            fprintf(stderr,
                    "fasta2fastq phases: files %.2f ms (waiting for blocks %.2f ms, device calls %.2f ms, to the writer %.2f ms, line-by-line loop %.2f ms), "
                    "closing the output %.2f ms; on the stream: text kernels %lld chunks %.3f ms\n",
                    (tc0 - t_start) * 1e3, c.t_read * 1e3, c.t_dev * 1e3, c.t_emit * 1e3, c.t_cpu * 1e3, (now_s() - tc0) * 1e3, (long long)n[2], ms[2]);
        }
        records = c.records;
    }
    if (!err && !wrote) err = hfail(GS_E_IO, std::string("writing ") + out_path + " failed");
    if (n_records) *n_records = records;
    return !err && stopped ? cancelled_rc() : err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- krakencount (C/goals/kraken/KrakenResCountGoal.java:133-157)
// ---- What the line-catalog goals share (krakencount, accmap, asmsum, taxtree): files of lines, chunks of whole lines to
// the device, what it refuses through the goal's exact parser at its place in the input order.  One loop of each kind over a per-goal
// struct G, whose members are the contract of the next such goal:
//   G::Reader                     how lines_cpu reads a file: WholeLines or RawPieces
//   begin_file(f)                 a file is a stream of its own: the parser's state, and where the file's line count starts
//   on_device(f)                  false: the file goes line by line although the call runs on a device
//   submit(path, cut, &refused)   a chunk to the device; one it took is booked here
//   feed(path, p, n, last)        whole lines through the host parser, and what it made of them into the handle
//   file_lines()                  the lines of the current file that are in the state: the count of its progress records
//   ended()                       the stream ends in front of the end of its file
//   end_file(f, path)             behind a file that went through without an error or a stop
namespace {

struct LineGoal {  // the base of every G: its counters, and the answers most goals give
    int64_t device_chunks = 0, host_chunks = 0;
    int prog_file = 0;  // progress records: the file being read
    bool on_device(int) const { return true; }
    bool ended() const { return false; }
    int end_file(int, const std::string &) { return GS_OK; }
};

// after a chunk; true: stop -- the chunk is in the state, the record of the stop is out
template <class G>
bool report(G &g, int64_t pos, bool gz) {
    if (!trk().chunk(g.prog_file, pos, gz, g.file_lines())) return false;
    trk().stopped(g.prog_file, g.file_lines());
    return true;
}

// The two ways lines_cpu reads a file from `offset` on.  next() makes [data(), data() + size()) the next piece of the stream and sets
// *eof with its last one; pos(): how far the file has been read, in its stored bytes.
struct WholeLines {  // whole lines, some MiB at a time, NUL bytes dropped (LineReader)
    LineReader lr;
    std::vector<uint8_t> text;
    int open(const std::string &path, int64_t offset) { return lr.open(path, offset) ? (int)GS_OK : hfail(GS_E_IO, "cannot open " + path); }
    int next(const std::string &, bool *eof) {
        text.clear();
        while (text.size() < ((size_t)4 << 20)) {
            if (lr.next_line(text) == 0) {
                *eof = true;
                break;
            }
        }
        // (next_line drops NUL bytes as the parser would; a final line without its newline is the stream's last)
        if (!text.empty() && text.back() != '\n') *eof = true;
        return GS_OK;
    }
    const uint8_t *data() const { return text.data(); }
    size_t size() const { return text.size(); }
    int64_t pos() const { return lr.raw_pos(); }
};
struct RawPieces {  // the text as it is, GS_HOST_BLOCK_BYTES at a time: NUL bytes are data, and the parser sees every CR
    gzFile gz = nullptr;
    std::vector<uint8_t> text;
    size_t n = 0;
    ~RawPieces() {
        if (gz) gzclose(gz);
    }
    int open(const std::string &path, int64_t offset) {
        gz = gzopen(path.c_str(), "rb");  // (zlib reads plain files transparently, gzip by content, member after member)
        if (!gz) return hfail(GS_E_IO, "cannot open " + path);
        gzbuffer(gz, 1 << 20);
        if (offset != 0 && gzseek(gz, (z_off_t)offset, SEEK_SET) != (z_off_t)offset) return hfail(GS_E_IO, "cannot seek in " + path);
        size_t piece = (size_t)4 << 20;
        if (const char *e = getenv("GS_HOST_BLOCK_BYTES")) piece = (size_t)std::max<long long>(1, atoll(e));
        text.resize(piece);
        return GS_OK;
    }
    int next(const std::string &path, bool *eof) {
        const int got = gzread(gz, text.data(), (unsigned)text.size());
        if (got < 0) return hfail(GS_E_IO, "cannot read " + path);
        n = (size_t)got;
        *eof = got == 0;
        return GS_OK;
    }
    const uint8_t *data() const { return text.data(); }
    size_t size() const { return n; }
    int64_t pos() const { return (int64_t)gzoffset(gz); }
};

// the rest of a stream through the host parser: the file from `offset` on (in its text), or a memory range that ends the stream
template <class G>
int lines_cpu(G &g, const std::string &path, int64_t offset, const uint8_t *mem, size_t mem_n) {
    g.host_chunks++;
    if (mem) {
        const int err = g.feed(path, mem, mem_n, true);
        return err ? err : report(g, 0, false) ? cancelled_rc() : (int)GS_OK;
    }
    typename G::Reader rd;
    int err = rd.open(path, offset);
    for (bool eof = false; !err && !eof && !g.ended();) {
        if ((err = rd.next(path, &eof))) break;
        err = g.feed(path, rd.data(), rd.size(), eof);
        if (!err && report(g, rd.pos(), false)) err = cancelled_rc();
    }
    return err;
}

// One file through the device: chunks that end behind a newline go there; one that the device refuses goes through the host parser,
// so the input order stays, and the stream goes on behind it on the device.  A line that does not fit a block sends the rest of the
// file through that parser; so does the unterminated tail.
template <class G>
int lines_device_file(G &g, const std::string &path, bool gzip) {
    size_t block;
    int readers = 0;
    reader_shape(gzip, &block, &readers);
    TextReader tr;
    int err = tr.open(path, block, readers, gzip);
    if (err) {
        tr.close();
        return err;
    }
    ChunkCutter cut;
    cut.mode = ChunkCutter::LINES;
    int64_t fallback_off = -1;
    tr.start();
    for (int64_t i = 0; !err; i++) {
        TextSlot &sl = tr.wait_full(i);
        if ((err = block_error(tr, sl, path))) break;
        const bool eof = sl.eof;
        const ChunkCutter::Cut what = cut_block(cut, tr, sl);
        if (what == ChunkCutter::FALLBACK) {
            fallback_off = cut.file_off;
        } else if (what == ChunkCutter::CHUNK && cut.bytes > 0) {
            bool refused = false;
            if ((err = g.submit(path, cut, &refused))) break;
            if (refused) {  // this chunk through the host parser
                g.host_chunks++;
                err = g.feed(path, cut.start, (size_t)cut.bytes, false);
            } else {
                g.device_chunks++;
            }
            cut.commit();
            if (!err && report(g, cut.file_off, gzip)) err = cancelled_rc();  // (the record is out: the block may go back)
        } else if (what == ChunkCutter::CHUNK) {
            cut.commit();
        }
        tr.release(i);
        if (eof || fallback_off >= 0 || g.ended()) break;
    }
    tr.close();
    if (err || g.ended()) return err;
    if (fallback_off >= 0) return lines_cpu(g, path, fallback_off, nullptr, 0);
    if (!cut.carry.empty()) return lines_cpu(g, path, 0, cut.carry.data(), cut.carry.size());
    return GS_OK;
}

// the files of a call, one after the other, under its progress records: GS_OK, GS_E_CANCELLED (the record of the stop is out) or
// what went wrong.  fast: chunks go to a device
template <class G>
int lines_files(G &g, const char *const *paths, int n_paths, bool fast) {
    int err = GS_OK;
    TrackerScope progress(paths, n_paths);
    Tracker &tk = progress.t;
    for (int f = 0; f < n_paths && !err; f++) {
        const std::string path(paths[f]);
        g.prog_file = f;
        g.begin_file(f);
        if (tk.file_start(f)) {
            tk.stopped(f, 0);
            err = cancelled_rc();
            break;
        }
        const int kind = fast && g.on_device(f) ? text_path_kind(path) : 0;
        err = kind ? lines_device_file(g, path, kind == 2 || kind == 4) : lines_cpu(g, path, 0, nullptr, 0);
        if (!err && tk.file_end(f, g.file_lines())) err = cancelled_rc();
        if (!err) err = g.end_file(f, path);
    }
    if (!err && tk.close()) err = cancelled_rc();
    return err;
}

}  // namespace

// ---- krakencount (C/goals/kraken/KrakenResCountGoal.java:133-157)
namespace {

struct KcGoal : LineGoal {
    using Reader = WholeLines;
    gs_krakencount *kc = nullptr;
    KrakenExact exact;  // rows of what the line-by-line loop took; its lines / tokens
    int64_t dev_tot[4] = {0, 0, 0, 0};
    int64_t prog_lines0 = 0;  // the lines counted when the file began
    int64_t file_lines() const { return exact.lines + dev_tot[0] - prog_lines0; }
    bool ended() const { return exact.ended; }  // an empty line: the stream ends there
    void begin_file(int) {  // every file is a stream of its own, all of them count into one table
        exact.ended = false;
        exact.line_no = 0;
        exact.forget_class();
        prog_lines0 = exact.lines + dev_tot[0];
    }
    int feed(const std::string &path, const uint8_t *p, size_t n, bool last) {
        if (exact.feed(p, n, last)) return GS_OK;
        return hfail(GS_E_INVALID, path + ": line " + std::to_string((long long)exact.line_no) + ": " + exact.error);
    }
    int submit(const std::string &, const ChunkCutter &cut, bool *refused) {
        int64_t ticket = 0, rep[8];
        if (gs_krakencount_submit(kc, cut.start, cut.bytes, GS_MEM_HOST, &ticket) != GS_OK || gs_krakencount_chunk(kc, ticket, rep) != GS_OK)
            return hfail(GS_E_HIP, gs_last_error());
        if ((*refused = rep[0] != 0)) return GS_OK;
        g_krakencount_chunks++;
        for (int j = 0; j < 4; j++) dev_tot[j] += rep[4 + j];
        if (rep[2] >= 0) {
            exact.ended = true;
        } else {
            exact.line_no += cut.lines;
            // (a later line without a class field has the class of the line before it, wherever that line was counted)
            const uint8_t *e = cut.start + cut.bytes - 1, *b = e;
            while (b > cut.start && b[-1] != '\n') b--;
            exact.set_class_of(b, (size_t)(e - b));
        }
        return GS_OK;
    }
};

}  // namespace

extern "C" int gs_host_kraken_count_files(int device, const char *const *paths, int n_paths, const char *const *only_taxids, int n_only,
                                          const char *csv_path, char *keys, int32_t key_stride, int64_t *counts, int64_t cap_rows, int64_t *n_rows,
                                          gs_host_kraken_totals *totals) try {
    if (!paths || n_paths < 0 || !n_rows || n_only < 0 || (n_only > 0 && !only_taxids)) return hfail(GS_E_INVALID, "NULL argument");
    *n_rows = 0;
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    int64_t max_taxids = (int64_t)1 << 18;
    if (const char *e = getenv("GS_KRAKEN_MAX_TAXIDS")) max_taxids = std::max<long long>(1, atoll(e));
    const double t_start = now_s();
    KcGoal c;
    HandleGuard<gs_krakencount, gs_krakencount_destroy> guard{c.kc};
    c.exact.filtered = n_only > 0;
    if (fast && gs_krakencount_create(&c.kc, device, max_taxids) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
    const int walked = lines_files(c, paths, n_paths, fast);
    // a stop on request: the rows of the lines counted so far are fetched all the same, no CSV is written
    const bool stopped = walked == GS_E_CANCELLED;
    if (walked && !stopped) return walked;
    std::map<std::string, KrakenRow> rows = c.exact.rows;
    if (c.kc) {
        int64_t n = 0;
        if (gs_krakencount_fetch(c.kc, nullptr, nullptr, 0, &n) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        std::vector<int32_t> ids((size_t)n + 1);
        std::vector<int64_t> cnt(3 * (size_t)n + 3);
        if (gs_krakencount_fetch(c.kc, ids.data(), cnt.data(), n, &n) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        for (int64_t i = 0; i < n; i++) {  // a device row's key is its decimal string
            KrakenRow &r = rows[std::to_string(ids[(size_t)i])];
            r.reads += cnt[3 * (size_t)i];
            r.kmers += cnt[3 * (size_t)i + 1];
            r.kimr += cnt[3 * (size_t)i + 2];
        }
    }
    if (n_only > 0) {
        std::map<std::string, KrakenRow> kept;
        for (int i = 0; i < n_only; i++) {
            if (!only_taxids[i]) return hfail(GS_E_INVALID, "NULL tax id");
            const auto it = rows.find(only_taxids[i]);
            if (it != rows.end()) kept.insert(*it);
        }
        rows.swap(kept);
    }
    if (totals) {
        totals->lines = c.exact.lines + c.dev_tot[0];
        totals->counted_tokens = c.exact.counted + c.dev_tot[1];
        totals->a_tokens = c.exact.a_tokens + c.dev_tot[2];
        totals->long_lines = c.exact.long_lines + c.dev_tot[3];
        totals->device_chunks = c.device_chunks;
        totals->host_chunks = c.host_chunks;
    }
    *n_rows = (int64_t)rows.size();
    size_t longest = 0;
    for (const auto &kv : rows) longest = std::max(longest, kv.first.size());
    std::vector<char> k2;
    std::vector<int64_t> c2;
    const int32_t stride = (int32_t)longest + 1;
    if (csv_path && !stopped) {
        k2.assign(rows.size() * (size_t)stride + 1, 0);
        c2.reserve(3 * rows.size() + 3);
        size_t i = 0;
        for (const auto &kv : rows) {
            memcpy(k2.data() + i++ * (size_t)stride, kv.first.data(), kv.first.size());
            c2.insert(c2.end(), {kv.second.reads, kv.second.kmers, kv.second.kimr});
        }
        const int err = gs_host_write_kraken_csv(csv_path, k2.data(), stride, c2.data(), (int64_t)rows.size());
        if (err) return err;
    }
    if (totals) totals->seconds_total = now_s() - t_start;
    if (cap_rows < *n_rows || (!rows.empty() && (!keys || !counts || (size_t)key_stride <= longest)))
        return hfail(GS_E_INVALID, "no room for " + std::to_string((long long)*n_rows) + " rows with keys of up to " + std::to_string(longest) + " bytes");
    size_t i = 0;
    for (const auto &kv : rows) {
        char *k = keys + i * (size_t)key_stride;
        memset(k, 0, (size_t)key_stride);
        memcpy(k, kv.first.data(), kv.first.size());
        counts[3 * i] = kv.second.reads;
        counts[3 * i + 1] = kv.second.kmers;
        counts[3 * i + 2] = kv.second.kimr;
        i++;
    }
    return stopped ? cancelled_rc() : (int)GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- RefSeq catalog files to the accession map (AccessionFileProcessor.processCatalog under AccessionMapSizeGoal / AccessionMapGoal;
// gs_accmap on the device, gs_accmapparse.h for what it refuses)
namespace {

struct AmGoal : LineGoal {
    using Reader = WholeLines;
    gs_accmap *am = nullptr;  // the device's map, or (GS_HOST_FAST=0) a host-only one
    bool keep = true;         // count_only == 0: entries go into am
    AccmapExact exact;        // the line-by-line parser: its buffer and line number live across a file
    int64_t flushed_passing = 0, dev_lines = 0;
    gs_host_accmap_totals tot{};
    int64_t prog_lines0 = 0;
    std::vector<uint8_t> slots;
    std::vector<int32_t> nodes;
    int64_t lines() const { return exact.lines + dev_lines; }
    int64_t file_lines() const { return lines() - prog_lines0; }
    void begin_file(int) {  // every file is a stream of its own, all of them go into one map
        exact.begin_stream();
        prog_lines0 = lines();
    }
    // what the parser has made since the last call goes into the map, in input order
    int flush(const std::string &path) {
        const int64_t passing = exact.passing - flushed_passing;
        flushed_passing = exact.passing;
        tot.passing += passing;
        tot.put += (int64_t)exact.entries.size();
        if (keep) {
            const size_t n = exact.entries.size();
            slots.assign(32 * n + 32, 0);
            nodes.assign(n + 1, 0);
            for (size_t i = 0; i < n; i++) {
                const std::string &key = exact.entries[i].key;
                bool fits = key.size() <= 31;
                for (unsigned char b : key) fits = fits && b < 0x80;
                if (!fits) return hfail(GS_E_UNSUPPORTED, path + ": the accession '" + key + "' does not fit a key slot (31 bytes below 0x80)");
                slots[32 * i] = (uint8_t)key.size();
                memcpy(slots.data() + 32 * i + 1, key.data(), key.size());
                nodes[i] = exact.entries[i].node;
            }
            if (gs_accmap_append(am, slots.data(), nodes.data(), (int64_t)n, passing) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        }
        exact.entries.clear();
        return GS_OK;
    }
    int feed(const std::string &path, const uint8_t *p, size_t n, bool last) {
        if (!exact.feed(p, n, last)) return hfail(GS_E_INVALID, path + ": line " + std::to_string((long long)exact.line_no) + ": " + exact.error);
        return flush(path);
    }
    int submit(const std::string &, const ChunkCutter &cut, bool *refused) {
        int64_t rep[8];
        if (gs_accmap_submit(am, cut.start, cut.bytes, GS_MEM_HOST, 0, rep) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        if ((*refused = rep[3] != 0)) return GS_OK;
        dev_lines += rep[0];
        tot.passing += rep[1];
        tot.put += rep[2];
        exact.line_no += rep[0];
        exact.note_chunk(cut.start, (size_t)cut.bytes);  // (a later line of fewer than five tabs reads what these left behind)
        return GS_OK;
    }
};

}  // namespace

extern "C" int gs_host_accmap_files(const char *const *paths, int n_paths, int device, const gs_accmap_cfg *cfg, int count_only, gs_accmap **out,
                                    gs_host_accmap_totals *totals) try {
    if (out) *out = nullptr;
    if (!paths || n_paths < 0 || !cfg || (!count_only && !out)) return hfail(GS_E_INVALID, "NULL argument");
    for (int f = 0; f < n_paths; f++)
        if (!paths[f]) return hfail(GS_E_INVALID, "NULL path");
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    const double t_start = now_s();
    AmGoal c;
    HandleGuard<gs_accmap, gs_accmap_destroy> guard{c.am};
    c.keep = !count_only;
    // (the handle checks cfg; a host-only one, device -1, touches no device)
    if (const int rc = gs_accmap_create(&c.am, fast ? device : -1, cfg)) return hfail(rc, gs_last_error());
    c.exact.dna = cfg->dna != 0;
    c.exact.rna = cfg->rna != 0;
    c.exact.mrna = cfg->mrna != 0;
    c.exact.categories.assign(cfg->categories, cfg->categories + cfg->n_categories);
    c.exact.statuses.assign(cfg->statuses, cfg->statuses + cfg->n_statuses);
    if (cfg->n_nodes) c.exact.known.assign(cfg->known_taxids, cfg->known_taxids + cfg->n_nodes);
    const int err = lines_files(c, paths, n_paths, fast);
    c.tot.lines = c.lines();
    c.tot.device_chunks = c.device_chunks;
    c.tot.host_chunks = c.host_chunks;
    if (!err && !count_only) {
        int64_t info[4];
        if (gs_accmap_finish(c.am, info) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        *out = c.am;
        c.am = nullptr;  // (the caller's now)
    }
    if (totals) {
        c.tot.seconds_total = now_s() - t_start;
        *totals = c.tot;
    }
    return err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- Genbank assembly summary files to the picks per node (AssemblySummaryReader.getRelevantEntries under FastaFilesFromGenbankGoal;
// gs_asmsum on the device, gs_asmsumparse.h for what it refuses)
namespace {

struct AsGoal : LineGoal {
    using Reader = RawPieces;  // NUL bytes are data here, and CR ends a line
    gs_asmsum *as = nullptr;   // the device's handle, or (GS_HOST_FAST=0) a host-only one
    AsmsumExact exact;         // the record-by-record parser: its line number is the current file's
    int64_t file_line0 = 0;    // the lines of the files in front of it
    int64_t flushed_counted = 0, flushed_lines = 0;
    gs_host_asmsum_totals tot{};
    std::vector<int32_t> nodes;
    std::vector<uint8_t> quality, is_ref, pool;
    std::vector<int64_t> lines;
    std::vector<uint64_t> str_off;
    int64_t file_lines() const { return exact.line_no; }
    void begin_file(int) {  // every file is a stream of its own, all of them go into one handle
        file_line0 += exact.line_no;
        exact.begin_stream();
        flushed_lines = 0;
    }
    // what the parser has made since the last call goes into the handle, in input order
    int flush() {
        const size_t n = exact.entries.size();
        nodes.assign(n + 1, 0);
        quality.assign(n + 1, 0);
        is_ref.assign(n + 1, 0);
        lines.assign(n + 1, 0);
        str_off.assign(3 * n + 1, 0);
        pool.clear();
        for (size_t i = 0; i < n; i++) {
            const AsmsumEntry &e = exact.entries[i];
            nodes[i] = e.node;
            quality[i] = e.quality;
            is_ref[i] = e.is_ref;
            lines[i] = file_line0 + e.line;
            for (const std::string *s : {&e.taxid, &e.species, &e.ftp}) {
                pool.insert(pool.end(), s->begin(), s->end());
                str_off[3 * i + (s == &e.taxid ? 1 : s == &e.species ? 2 : 3)] = pool.size();
            }
        }
        pool.push_back(0);
        const int64_t counted = exact.counted - flushed_counted, n_lines = exact.line_no - flushed_lines;
        flushed_counted = exact.counted;
        flushed_lines = exact.line_no;
        tot.counted += counted;
        tot.kept += (int64_t)n;
        if (gs_asmsum_append(as, nodes.data(), quality.data(), is_ref.data(), lines.data(), str_off.data(), pool.data(), (int64_t)n, counted, n_lines) != GS_OK)
            return hfail(GS_E_HIP, gs_last_error());
        exact.entries.clear();
        return GS_OK;
    }
    int feed(const std::string &path, const uint8_t *p, size_t n, bool last) {
        if (!exact.feed(p, n, last)) return hfail(GS_E_INVALID, path + ": line " + std::to_string((long long)exact.line_no) + ": " + exact.error);
        return flush();
    }
    int submit(const std::string &, const ChunkCutter &cut, bool *refused) {
        int64_t rep[8];
        if (gs_asmsum_submit(as, cut.start, cut.bytes, GS_MEM_HOST, 0, rep) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        if ((*refused = rep[3] != 0)) return GS_OK;
        tot.counted += rep[0];
        tot.kept += rep[1];
        exact.line_no += rep[0] + rep[2] + rep[6];
        flushed_lines = exact.line_no;
        return GS_OK;
    }
};

}  // namespace

extern "C" int gs_host_asmsum_files(const char *const *paths, int n_paths, int device, const gs_asmsum_cfg *cfg, int32_t max_per_node, gs_asmsum **out,
                                    gs_host_asmsum_totals *totals) try {
    if (out) *out = nullptr;
    if (!paths || n_paths < 0 || !cfg || !out) return hfail(GS_E_INVALID, "NULL argument");
    for (int f = 0; f < n_paths; f++)
        if (!paths[f]) return hfail(GS_E_INVALID, "NULL path");
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    const double t_start = now_s();
    AsGoal c;
    HandleGuard<gs_asmsum, gs_asmsum_destroy> guard{c.as};
    // (the handle checks cfg; a host-only one, device -1, touches no device)
    if (const int rc = gs_asmsum_create(&c.as, fast ? device : -1, cfg)) return hfail(rc, gs_last_error());
    if (cfg->n_nodes) c.exact.known.assign(cfg->known_taxids, cfg->known_taxids + cfg->n_nodes);
    if (cfg->filter && cfg->n_nodes) c.exact.filter.assign(cfg->filter, cfg->filter + cfg->n_nodes);
    c.exact.quality_mask = cfg->quality_mask;
    c.exact.reference_only = cfg->reference_only != 0;
    c.exact.use_species = cfg->use_species_taxid != 0;
    const int err = lines_files(c, paths, n_paths, fast);
    c.tot.lines = c.file_line0 + c.exact.line_no;
    c.tot.device_chunks = c.device_chunks;
    c.tot.host_chunks = c.host_chunks;
    if (!err) {
        int64_t info[4];
        if (gs_asmsum_finish(c.as, max_per_node, info) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
        c.tot.picked = info[1];
        c.tot.nodes = info[2];
        *out = c.as;
        c.as = nullptr;  // (the caller's now)
    }
    if (totals) {
        c.tot.seconds_total = now_s() - t_start;
        *totals = c.tot;
    }
    return err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- NCBI taxonomy dump files to the tree (TaxTree(File, boolean); gs_taxtree on the device, gs_taxparse.h inside the handle for
// what the device refuses)
namespace {

struct TtGoal : LineGoal {
    using Reader = WholeLines;
    gs_taxtree *t = nullptr;
    int64_t *rep = nullptr;  // the call's report: what finish_nodes says goes there behind file 0
    bool names = false;      // the names stream: gs_taxtree_submit_names / _append_names
    bool finish_failed = false;
    int64_t lines = 0, prog_lines0 = 0;
    int64_t file_lines() const { return lines - prog_lines0; }
    void begin_file(int f) {
        names = f == 1;
        prog_lines0 = lines;
    }
    // (a tree that fell back to the host's lists -- duplicate ids -- takes its names line by line as well)
    bool on_device(int f) const { return f == 0 || rep[7] == 0; }
    // whole lines through the line-by-line restatement inside the handle, at their place in the input order
    int feed(const std::string &path, const uint8_t *p, size_t n, bool last) {
        if (names) {
            const int rc = gs_taxtree_append_names(t, p, (int64_t)n, last);
            if (rc != GS_OK) return hfail(rc, path + ": " + gs_last_error());
            lines += (int64_t)std::count(p, p + n, (uint8_t)'\n') + (n && p[n - 1] != '\n');
            return GS_OK;
        }
        int64_t r[8];
        const int rc = gs_taxtree_append_nodes(t, p, (int64_t)n, last, r);
        if (rc != GS_OK) return hfail(rc, path + ": " + gs_last_error());
        lines += r[0];
        return GS_OK;
    }
    int submit(const std::string &path, const ChunkCutter &cut, bool *refused) {
        int64_t r[8];
        const int rc = names ? gs_taxtree_submit_names(t, cut.start, cut.bytes, GS_MEM_HOST, 0, r) : gs_taxtree_submit_nodes(t, cut.start, cut.bytes, GS_MEM_HOST, 0, r);
        if (rc != GS_OK) return hfail(rc, path + ": " + gs_last_error());
        if (!(*refused = r[3] != 0)) lines += r[0];
        return GS_OK;
    }
    int end_file(int f, const std::string &path) {  // behind the nodes: the tree
        if (f != 0) return GS_OK;
        rep[0] = lines;
        int64_t info[8];
        const int rc = gs_taxtree_finish_nodes(t, info);
        if (rc != GS_OK) {
            finish_failed = true;
            return hfail(rc, path + ": " + gs_last_error());
        }
        rep[4] = info[0];
        rep[5] = info[1];
        rep[6] = info[3];
        rep[7] = info[4];
        return GS_OK;
    }
};

}  // namespace

extern "C" int gs_host_taxtree_files(int device, const char *nodes_path, const char *names_path, gs_taxtree **out, int64_t report[8]) try {
    if (out) *out = nullptr;
    if (!nodes_path || !out || !report) return hfail(GS_E_INVALID, "NULL argument");
    for (int i = 0; i < 8; i++) report[i] = 0;
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    TtGoal c;
    HandleGuard<gs_taxtree, gs_taxtree_destroy> guard{c.t};
    c.rep = report;
    if (const int rc = gs_taxtree_create(&c.t, fast ? device : -1)) return hfail(rc, gs_last_error());
    const char *paths[2] = {nodes_path, names_path};
    const int err = lines_files(c, paths, names_path ? 2 : 1, fast);
    if (c.finish_failed) return err;
    report[1] = c.lines - report[0];
    report[2] = c.device_chunks;
    report[3] = c.host_chunks;
    if (!err) {
        *out = c.t;
        c.t = nullptr;  // (the caller's now)
    }
    return err;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// TaxIdCollector.readFromFile: the file (plain or gzip) as bytes through gs_taxtree_read_taxids
extern "C" int gs_host_read_taxids_file(const char *path, int32_t *requested, int64_t *n_requested, int32_t *excluded, int64_t *n_excluded, int64_t cap) try {
    if (!path || !n_requested || !n_excluded || cap < 0) return hfail(GS_E_INVALID, "NULL or negative argument");
    LineReader lr;
    if (!lr.open(path, 0)) return hfail(GS_E_IO, std::string("cannot open ") + path);
    std::vector<uint8_t> text;
    while (lr.next_line(text) != 0) {
    }
    const int rc = gs_taxtree_read_taxids(text.data(), (int64_t)text.size(), requested, n_requested, excluded, n_excluded, cap);
    return rc ? hfail(rc, gs_last_error()) : (int)GS_OK;
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- genome FASTA files to regions (AbstractFastaReader.readFasta under the store readers; gs_genomes on the device)
namespace {

struct GnCtx {
    gs_genomes *g = nullptr;
    gs_genome_resolve_fn resolve = nullptr;
    gs_genome_sink_fn sink = nullptr;
    void *resolve_user = nullptr, *sink_user = nullptr;
    // gs_host_genome_files_mapped: the map looks the header lines up, the resolver sees one node per record
    gs_accmap *am = nullptr;
    int complete_only = 0;
    gs_genome_resolve_nodes_fn resolve_nodes = nullptr;
    const int32_t *node_of_file = nullptr;  // gs_host_genome_files_into: >= 0: the node of every record of that file, no lookup
    std::vector<int32_t> node;
    int file = 0;
    int64_t first_record = 0;  // records of the file in front of the chunk
    gs_host_genome_totals tot{};
    std::vector<uint8_t> hdr, keep, kseq;
    std::vector<uint64_t> hoff, koff;
    std::vector<int32_t> vi, kvi;
    GenomeRecords rec;
    // after a chunk whose regions the sink has taken; true: stop -- nothing is in flight (the sink has returned), the record is out
    bool report(int64_t pos, bool gz) {
        if (!trk().chunk(file, pos, gz, first_record)) return false;
        trk().stopped(file, first_record);
        return true;
    }
};

// the caller's decision for the n records of a chunk -> keep[n], kvi (vi of the kept ones); a callback's own code comes back as it is.
// With a map: hdr == nullptr says that the header lines are those of the chunk c.g has scanned, and stay on the device
int gn_resolve(GnCtx &c, int64_t n, const uint8_t *hdr, const uint64_t *hoff) {
    c.vi.assign((size_t)n, -1);
    c.keep.assign((size_t)n, 0);
    c.kvi.clear();
    if (n == 0) return 0;
    int rc;
    if (c.resolve_nodes) {
        const int32_t fixed = c.node_of_file ? std::max(c.node_of_file[c.file], -1) : -1;
        c.node.assign((size_t)n, fixed);
        rc = fixed >= 0 ? (int)GS_OK
             : hdr      ? gs_accmap_lookup(c.am, hdr, hoff, n, GS_MEM_HOST, c.complete_only, c.node.data())
                        : gs_accmap_lookup_genomes(c.am, c.g, c.complete_only, c.node.data());
        if (rc) return hfail(rc, gs_last_error());
        rc = c.resolve_nodes(c.resolve_user, c.file, c.first_record, n, c.node.data(), c.vi.data());
    } else {
        rc = c.resolve(c.resolve_user, c.file, c.first_record, n, hdr, hoff, c.vi.data());
    }
    if (rc) return rc;
    for (int64_t i = 0; i < n; i++)
        if (c.vi[(size_t)i] >= 0) {
            c.keep[(size_t)i] = 1;
            c.kvi.push_back(c.vi[(size_t)i]);
        }
    c.first_record += n;
    c.tot.records += n;
    c.tot.kept_records += (int64_t)c.kvi.size();
    return 0;
}

// [p, p + n) line by line; last: the stream ends behind it.  *consumed: the bytes its whole records cover
int gn_host_chunk(GnCtx &c, const uint8_t *p, size_t n, bool last, size_t *consumed) {
    genome_parse(p, n, last, &c.rec);
    *consumed = c.rec.consumed;
    c.tot.chunks++;
    c.tot.host_chunks++;
    c.tot.text_bytes += (int64_t)c.rec.consumed;
    c.tot.max_line_bytes = std::max(c.tot.max_line_bytes, c.rec.max_line);
    const int64_t nr = c.rec.records();
    int rc = gn_resolve(c, nr, c.rec.headers.data(), c.rec.header_off.data());
    if (rc || c.kvi.empty()) return rc;
    c.kseq.clear();
    c.koff.assign(1, 0);
    for (int64_t i = 0; i < nr; i++)
        if (c.keep[(size_t)i]) {
            c.kseq.insert(c.kseq.end(), c.rec.seq.begin() + (long)c.rec.off[(size_t)i], c.rec.seq.begin() + (long)c.rec.off[(size_t)i + 1]);
            c.koff.push_back(c.kseq.size());
        }
    c.tot.kept_bases += (int64_t)c.kseq.size();
    if (c.kseq.empty()) c.kseq.push_back(0);  // (regions of no bases: a pointer all the same)
    return c.sink(c.sink_user, c.kseq.data(), c.koff.data(), c.kvi.data(), (int64_t)c.kvi.size(), GS_MEM_HOST);
}

// a chunk of whole records through the device; refused (or larger than the device takes): line by line
int gn_chunk(GnCtx &c, const uint8_t *p, int64_t n) {
    int64_t nr = 0, used = 0, hb = 0, ml = 0;
    int rc = c.g ? gs_genomes_scan(c.g, p, n, GS_MEM_HOST, 1, &nr, &used, &hb, &ml) : (int)GS_E_UNSUPPORTED;
    if (rc == GS_E_UNSUPPORTED) {
        size_t all = 0;
        return gn_host_chunk(c, p, (size_t)n, true, &all);
    }
    if (rc) return hfail(rc, gs_last_error());
    c.tot.chunks++;
    c.tot.text_bytes += used;
    c.tot.max_line_bytes = std::max(c.tot.max_line_bytes, ml);
    if (c.resolve_nodes) {  // the header lines never leave the device
        if ((rc = gn_resolve(c, nr, nullptr, nullptr)) || c.kvi.empty()) return rc;
    } else {
        c.hdr.resize((size_t)hb + 1);
        c.hoff.resize((size_t)nr + 1);
        if ((rc = gs_genomes_headers(c.g, c.hdr.data(), c.hoff.data()))) return hfail(rc, gs_last_error());
        if ((rc = gn_resolve(c, nr, c.hdr.data(), c.hoff.data())) || c.kvi.empty()) return rc;
    }
    int64_t n_regions = 0, n_bases = 0;
    const uint8_t *d_seq = nullptr;
    const uint64_t *d_off = nullptr;
    if ((rc = gs_genomes_gather(c.g, c.keep.data(), &n_regions, &n_bases)) || (rc = gs_genomes_regions(c.g, &d_seq, &d_off)))
        return hfail(rc, gs_last_error());
    c.tot.kept_bases += n_bases;
    return c.sink(c.sink_user, d_seq, d_off, c.kvi.data(), n_regions, GS_MEM_DEVICE);
}

// the file from `offset` on (in its text), line by line: some MiB of whole lines at a time, cut in front of the buffer's last header
// line.  Where that line starts is noted as the lines come in, so a record of any length is looked at once, not once per turn.
int gn_host_stream(GnCtx &c, const std::string &path, int64_t offset) {
    LineReader lr;
    if (!lr.open(path, offset)) return hfail(GS_E_IO, "cannot open " + path);
    std::vector<uint8_t> text;
    size_t want = (size_t)4 << 20;
    for (bool eof = false; !eof;) {
        size_t last_hdr = 0;  // start of the last header line behind the buffer's first byte (0: none)
        while (text.size() < want) {
            const size_t at = text.size();
            if (lr.next_line(text) == 0) {
                eof = true;
                break;
            }
            if (at > 0 && text[at] == '>') last_hdr = at;
        }
        // the records that END in the buffer: all of it at the end of the stream, else what lies in front of its last header line;
        // without one the buffer is one record that goes on (more of it), or whole lines that belong to no record
        const size_t n = eof ? text.size() : last_hdr ? last_hdr : (!text.empty() && text[0] == '>') ? 0 : text.size();
        if (n > 0) {
            size_t used = 0;
            const int rc = gn_host_chunk(c, text.data(), n, true, &used);
            if (rc) return rc;
            if (c.report(lr.raw_pos(), false)) return cancelled_rc();
            text.erase(text.begin(), text.begin() + (long)n);
        }
        want = text.size() + ((size_t)4 << 20);
    }
    return GS_OK;
}

// One pass over a file with reader blocks of `block` bytes, for the records from text offset `from` on (a plain file is read from
// there; a gzip stream cannot be entered in the middle: it is inflated from its start and what lies in front of `from` -- whole
// records, worked off by an earlier pass -- is passed over).  The blocks are cut in front of their last header line, so a chunk is
// whole records and every one of them ends in it; what lies behind the last cut at the end of the file (no final newline) is one
// more chunk.  *fallback_off >= 0: a record that does not fit the headroom of a block starts there.
int gn_device_pass(GnCtx &c, const std::string &path, bool gzip, size_t block, int readers, int64_t from, int64_t *fallback_off) {
    TextReader tr;
    int err = tr.open(path, block, readers, gzip);
    if (err) {
        tr.close();
        return err;
    }
    const int64_t base = gzip ? 0 : from;  // text offset of the pass's first byte
    tr.start_off = base;
    ChunkCutter cut;
    cut.mode = ChunkCutter::FASTA;
    // [p, p + n) lies at text offset `at`: its part from `from` on (`from` is where a chunk of an earlier pass started: a header line)
    const auto chunk_from = [&](const uint8_t *p, int64_t n, int64_t at) {
        const int64_t d = std::min<int64_t>(std::max<int64_t>(from - at, 0), n);
        return n - d > 0 ? gn_chunk(c, p + d, n - d) : (int)GS_OK;
    };
    tr.start();
    for (int64_t i = 0; !err; i++) {
        TextSlot &sl = tr.wait_full(i);
        if ((err = block_error(tr, sl, path))) break;
        const bool eof = sl.eof;
        const ChunkCutter::Cut what = cut_block(cut, tr, sl);
        if (what == ChunkCutter::FALLBACK) {
            *fallback_off = std::max(from, base + cut.file_off);
        } else if (what == ChunkCutter::CHUNK) {
            err = chunk_from(cut.start, cut.bytes, base + cut.file_off);
            if (!err) cut.commit();
            if (!err && c.report(base + cut.file_off, gzip)) err = cancelled_rc();  // (the record is out: the block may go back)
        }
        tr.release(i);
        if (eof || *fallback_off >= 0) break;
    }
    tr.close();
    if (err || *fallback_off >= 0) return err;
    err = chunk_from(cut.carry.data(), (int64_t)cut.carry.size(), base + cut.file_off);
    if (!err && !cut.carry.empty() && c.report(base + cut.file_off, gzip)) err = cancelled_rc();
    return err;
}

// One file through the device.  A record longer than a block: the file goes on from that record with blocks twice as large, up to
// 512 MiB (a chunk -- the carry and a block -- holds at most 1 GiB); a record beyond that size is the line-by-line loop's, with the
// rest of its file.  The readers pin 2 x readers blocks of twice the block size (gzip: 4 of them): the readers of a plain file are
// cut down as the blocks grow so that they stay within 1 GiB of page-locked memory (2 GiB at 512 MiB; gzip: 0.5 GiB at the default
// block, 4 GiB at 512 MiB), and the idle blocks of the smaller size go back before a pass with larger ones starts.
int gn_device_file(GnCtx &c, const std::string &path, bool gzip) {
    size_t block;
    int readers = 0;
    reader_shape(gzip, &block, &readers);
    if (!getenv("GS_HOST_BLOCK_BYTES")) block = (size_t)64 << 20;  // (genomes, not reads: a record is megabytes)
    const size_t largest = (size_t)512 << 20;
    for (int64_t from = 0;;) {
        const int fit = (int)std::max<size_t>(1, ((size_t)256 << 20) / block);
        int64_t fallback_off = -1;
        const int err = gn_device_pass(c, path, gzip, block, gzip ? readers : std::min(readers, fit), from, &fallback_off);
        if (err || fallback_off < 0) return err;
        if (block >= largest) return gn_host_stream(c, path, fallback_off);
        block = std::min(block * 2, largest);
        from = fallback_off;
        gs_host::pinned_pool().release_all();  // (the readers' blocks: gs_ingest.h)
    }
}

}  // namespace

namespace {

// the walk over the files behind both front ends; c holds the resolver (header lines, or a map and nodes) and the sink
int gn_files(GnCtx &c, const char *const *paths, int n_paths, int device, gs_host_genome_totals *totals) {
    for (int f = 0; f < n_paths; f++)
        if (!paths[f]) return hfail(GS_E_INVALID, "NULL path");
    bool fast = true;
    if (const char *e = getenv("GS_HOST_FAST")) fast = atoi(e) != 0;
    const double t_start = now_s();
    HandleGuard<gs_genomes, gs_genomes_destroy> guard{c.g};
    if (fast && gs_genomes_create(&c.g, device) != GS_OK) return hfail(GS_E_HIP, gs_last_error());
    int err = GS_OK;
    TrackerScope progress(paths, n_paths);
    Tracker &tk = progress.t;
    for (int f = 0; f < n_paths && !err; f++) {
        const std::string path(paths[f]);
        c.file = f;
        c.first_record = 0;
        if (tk.file_start(f)) {
            tk.stopped(f, 0);
            err = cancelled_rc();
            break;
        }
        const int kind = fast ? text_path_kind(path) : 0;
        err = kind ? gn_device_file(c, path, kind == 2 || kind == 4) : gn_host_stream(c, path, 0);
        if (!err && tk.file_end(f, c.first_record)) err = cancelled_rc();
    }
    if (!err && tk.close()) err = cancelled_rc();
    c.tot.seconds_total = now_s() - t_start;
    if (totals) *totals = c.tot;
    return err;
}

}  // namespace

extern "C" int gs_host_genome_files(const char *const *paths, int n_paths, int device, gs_genome_resolve_fn resolve, void *resolve_user,
                                    gs_genome_sink_fn sink, void *sink_user, gs_host_genome_totals *totals) try {
    if (!paths || n_paths < 0 || !resolve || !sink) return hfail(GS_E_INVALID, "NULL argument");
    GnCtx c;
    c.resolve = resolve;
    c.resolve_user = resolve_user;
    c.sink = sink;
    c.sink_user = sink_user;
    return gn_files(c, paths, n_paths, device, totals);
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

extern "C" int gs_host_genome_files_mapped(const char *const *paths, int n_paths, int device, gs_accmap *am, int complete_only,
                                           gs_genome_resolve_nodes_fn resolve, void *resolve_user, gs_genome_sink_fn sink, void *sink_user,
                                           gs_host_genome_totals *totals) try {
    if (!paths || n_paths < 0 || !am || !resolve || !sink) return hfail(GS_E_INVALID, "NULL argument");
    GnCtx c;
    c.am = am;
    c.complete_only = complete_only;
    c.resolve_nodes = resolve;
    c.resolve_user = resolve_user;
    c.sink = sink;
    c.sink_user = sink_user;
    return gn_files(c, paths, n_paths, device, totals);
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}

// ---- gs_host_genome_files_into: the loop of gs_host_genome_files_mapped with the common resolver and sink built in
namespace {

struct GnInto {
    const int32_t *vi_of_node = nullptr;
    int32_t n_nodes = 0;
    int kind = 0, update = 0;
    void *handle = nullptr;
};

int gn_into_resolve(void *user, int, int64_t, int64_t n, const int32_t *node, int32_t *vi) {
    const GnInto &t = *static_cast<const GnInto *>(user);
    for (int64_t i = 0; i < n; i++) vi[i] = node[i] >= 0 && node[i] < t.n_nodes ? std::max(t.vi_of_node[node[i]], -1) : -1;
    return 0;
}

int gn_into_sink(void *user, const uint8_t *seq, const uint64_t *off, const int32_t *vi, int64_t n_regions, int mem) {
    const GnInto &t = *static_cast<const GnInto *>(user);
    int rc = GS_E_INVALID;
    switch (t.kind) {
    case GS_HOST_INTO_SIZE: rc = gs_dbsize_add(static_cast<gs_dbsize *>(t.handle), seq, off, vi, n_regions, mem); break;
    case GS_HOST_INTO_BUILD: rc = gs_dbbuild_add(static_cast<gs_dbbuild *>(t.handle), seq, off, vi, n_regions, mem, t.update); break;
    case GS_HOST_INTO_UPDATE: rc = gs_dbupdate_add(static_cast<gs_dbupdate *>(t.handle), seq, off, vi, n_regions, mem); break;
    case GS_HOST_INTO_QUALITY: rc = gs_dbquality_add(static_cast<gs_dbquality *>(t.handle), seq, off, vi, n_regions, mem); break;
    }
    return rc ? hfail(rc, gs_last_error()) : 0;
}

}  // namespace

extern "C" int gs_host_genome_files_into(const char *const *paths, int n_paths, int device, gs_accmap *am, int complete_only,
                                         const int32_t *node_of_file, const int32_t *vi_of_node, int32_t n_nodes, int kind, void *handle,
                                         int update, gs_host_genome_totals *totals) try {
    if (!paths || n_paths < 0 || n_nodes < 0 || (n_nodes > 0 && !vi_of_node)) return hfail(GS_E_INVALID, "NULL or negative argument");
    if (!handle) return hfail(GS_E_INVALID, "NULL target handle");
    if (kind != GS_HOST_INTO_SIZE && kind != GS_HOST_INTO_BUILD && kind != GS_HOST_INTO_UPDATE && kind != GS_HOST_INTO_QUALITY)
        return hfail(GS_E_INVALID, "unknown target kind " + std::to_string(kind));
    if (am) {
        int32_t map_nodes = -1;
        const int rc = gs_accmap_get_n_nodes(am, &map_nodes);
        if (rc) return hfail(rc, gs_last_error());
        if (map_nodes != n_nodes)
            return hfail(GS_E_INVALID, "vi_of_node has " + std::to_string(n_nodes) + " nodes, the accession map " + std::to_string(map_nodes));
    }
    for (int f = 0; f < n_paths; f++) {
        const int32_t fixed = node_of_file ? node_of_file[f] : -1;
        if (fixed < 0 && !am) return hfail(GS_E_INVALID, "file " + std::to_string(f) + " needs a lookup and there is no accession map");
        if (fixed >= n_nodes) return hfail(GS_E_INVALID, "node_of_file[" + std::to_string(f) + "] is no node");
    }
    GnInto t;
    t.vi_of_node = vi_of_node;
    t.n_nodes = n_nodes;
    t.kind = kind;
    t.update = update ? 1 : 0;
    t.handle = handle;
    GnCtx c;
    c.am = am;
    c.complete_only = complete_only;
    c.node_of_file = node_of_file;
    c.resolve_nodes = gn_into_resolve;
    c.resolve_user = &t;
    c.sink = gn_into_sink;
    c.sink_user = &t;
    return gn_files(c, paths, n_paths, device, totals);
} catch (const std::bad_alloc &) {
    return hfail(GS_E_NOMEM, "out of host memory");
} catch (const std::exception &e) {
    return hfail(GS_E_INVALID, std::string("unexpected exception: ") + e.what());
}
