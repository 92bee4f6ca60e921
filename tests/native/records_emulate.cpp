// records_emulate.cpp -- the text kernels of genestrip_amd/csrc/gs_rewrite.hip for the records of FASTA and general FASTQ chunks
// (descriptor lines, the gather of the quality lines, sizes, offsets, pieces, the copy) and the record instantiation of the
// Kraken-style kernels of gs_kraken.hip, compiled for the host against a stand-in for the few HIP constructs they use (a block is
// 256 real threads, tests/native/kraken_emulate_hip.h) and run under AddressSanitizer / UBSan.  The text must equal a plain
// formatter's byte for byte, and the bytes in front of the output and behind its last 16-byte word must stay untouched.
// Shapes: FASTA with header-only records at the start, in the middle and at the end; general FASTQ with 1 .. 3 sequence lines,
// qualities over another number of lines, a last quality line that overshoots, CRLF, descriptors of one byte and of none, half a
// record behind the last whole one; every selection (none, all, first, last, masks); 255 / 256 / 257 / 513 records; descriptor
// lengths 1 .. 17; a record of more than two pieces; totals around 4096 and 8192 bytes.
// The test that builds it (tests/test_record_text_cpu.py) puts a <hip/hip_runtime.h> that includes records_emulate_hip.h on the
// include path.
#include "records_emulate_hip.h"
thread_local dim3 threadIdx, blockIdx;
dim3 gridDim;
std::barrier<> *g_block_bar;
std::barrier<> *g_wave_bar[4];
unsigned long long g_xch[4][64];
typedef unsigned long long u64;
#include "../../genestrip_amd/csrc/gs_rewrite.hip"
#include "../../genestrip_amd/csrc/gs_kraken.hip"
#include <stdio.h>
#include <random>
#include <string>

struct Rec {
    std::string desc;
    std::vector<std::string> seq, qual;  // lines without their '\n'
};
struct Chunk {
    bool fasta = false;
    std::vector<Rec> recs;
    std::string tail;  // half a record behind the last whole one (general FASTQ)
};

static int g_fails = 0;

static std::string letters(std::mt19937_64 &rng, size_t n, const char *abc, size_t m) {
    std::string s(n, ' ');
    for (auto &c : s) c = abc[rng() % m];
    return s;
}

// one chunk through the kernels: record text under (flags, mask, want, probs) and Kraken-style lines at k, write_all
static void run(const char *name, const Chunk &ch, const std::vector<uint8_t> &flags, uint32_t mask, uint32_t want, bool probs, int k, int write_all,
                std::mt19937_64 &rng) {
    // the chunk as the text stage leaves it: text, newline offsets, line classes, the reads gathered, their bounds, the scan words
    std::string text;
    std::vector<uint32_t> nl;
    std::vector<uint8_t> cls;
    std::string seq;
    std::vector<u64> off2{0};
    auto line = [&](const std::string &s, uint8_t c) {
        text += s;
        nl.push_back((uint32_t)text.size());
        text += '\n';
        cls.push_back(c);
    };
    for (const Rec &r : ch.recs) {
        line(r.desc, 1);
        for (auto &s : r.seq) {
            line(s, 2);
            seq += s;
        }
        off2.push_back(seq.size());
        if (!ch.fasta) {
            line("+", 0);
            for (auto &q : r.qual) line(q, 0);
        }
    }
    const int64_t n_lines = (int64_t)nl.size(), n = (int64_t)ch.recs.size();
    for (size_t a = 0; a < ch.tail.size();) {  // lines the records do not cover: in nl[] behind n_lines
        const size_t b = ch.tail.find('\n', a);
        text += ch.tail.substr(a, b - a);
        nl.push_back((uint32_t)text.size());
        text += '\n';
        cls.push_back(0);
        a = b + 1;
    }
    text += std::string(64, ' ');
    const int64_t n_blocks = (n_lines + 255) / 256;
    std::vector<u64> fa_scan(n_lines + 1), fa_block(n_blocks + 2);
    u64 run_all = 0;
    for (int64_t b = 0; b < n_blocks; b++) {
        u64 in = 0;
        for (int64_t i = b * 256; i < std::min<int64_t>(n_lines, b * 256 + 256); i++) {
            fa_scan[i] = in;
            const uint32_t start = i ? nl[i - 1] + 1 : 0;
            in += cls[i] == 1 ? RW_HDR : (cls[i] == 2 ? nl[i] - start : 0);
        }
        fa_block[b] = run_all;
        run_all += in;
    }
    uint32_t status[GS_TS_WORDS] = {0, 0, 0xffffffffu, 0, 0, 0, 0, 0};
    std::vector<uint32_t> rec_line(n + 1, 0xdeadbeefu), piece(text.size() * 2 / 4096 + 8), q_dst(n_lines + 1);
    std::vector<u64> rec_out(n + 1), rec_block(n / 256 + 2), q_scan(n_lines + 1), q_block(n_blocks + 2), q_off(n + 1);
    std::vector<uint8_t> q_seq(text.size() + 256, 0xCC);
    u64 totals[4] = {0, 0, 0, 0};
    GsRewriteParams R{};
    R.text = (const uint8_t *)text.data();
    R.n_lines = n_lines;
    R.n_records = n;
    R.nl = nl.data();
    R.line_class = ch.fasta ? nullptr : cls.data();
    R.fa_scan = fa_scan.data();
    R.fa_block = fa_block.data();
    R.fa_seq = (uint8_t *)seq.data();
    R.off2 = off2.data();
    R.status = status;
    R.gate = status + GS_TS_SKIP;
    R.keep_first = ch.fasta ? 0 : 1;
    R.rec_line = rec_line.data();
    R.rec_out = rec_out.data();
    R.rec_block = rec_block.data();
    R.piece_rec = piece.data();
    R.totals = totals;
    const bool quals = probs && !ch.fasta;
    if (quals) {
        GsRewriteParams Q = R;
        Q.goal_mode = 2;
        Q.fa_scan = q_scan.data();
        Q.fa_block = q_block.data();
        Q.line_dst = q_dst.data();
        Q.fa_seq = q_seq.data();
        Q.off2 = q_off.data();
        gs_launch_rewrite_lines(&Q, nullptr);
        R.q_seq = q_seq.data();
        R.q_off = q_off.data();
    } else
        gs_launch_rewrite_heads(&R, nullptr);
    totals[0] = totals[1] = totals[2] = totals[3] = 0;
    // what a plain formatter writes
    std::string expect;
    u64 expect_n = 0;
    for (int64_t r = 0; r < n; r++) {
        if (!flags.empty() && (uint32_t)((flags[r] & mask) != 0) != want) continue;
        const Rec &c = ch.recs[r];
        std::string d = c.desc, s, q;
        if (ch.fasta && !d.empty()) d[0] = '@';
        for (auto &x : c.seq) s += x;
        for (auto &x : c.qual) q += x;
        expect += d + "\n" + s + "\n+\n" + (quals ? q : std::string(s.size(), '~')) + "\n";
        expect_n++;
    }
    const size_t bound = ((2 * text.size() + 5 * (size_t)n + 15) & ~(size_t)15) + 64;
    std::vector<uint8_t> outbuf(bound + 64, 0xEE);
    uint8_t *base = outbuf.data();
    while (((uintptr_t)base & 15) != 0) base++;
    base += 16;
    R.flags = flags.empty() ? nullptr : flags.data();
    R.flag_mask = mask;
    R.flag_want = want;
    R.out = base;
    gs_launch_rewrite_copy(&R, (int64_t)bound - 64, 4, nullptr);
    const size_t end = ((size_t)totals[0] + 15) & ~(size_t)15;  // (the copy stores whole 16-byte words)
    bool ok = totals[0] == expect.size() && totals[1] == expect_n && memcmp(base, expect.data(), expect.size()) == 0;
    for (int i = 1; i <= 16; i++) ok = ok && base[-i] == 0xEE;
    for (size_t i = end; i < end + 32; i++) ok = ok && base[i] == 0xEE;
    for (int64_t r = 0; r <= n; r++) ok = ok && rec_line[r] != 0xdeadbeefu;
    ok = ok && rec_line[n] == (uint32_t)n_lines;
    printf("%-34s records %5lld probs %d mask %3u want %u: bytes %llu (want %zu) records %llu (want %llu) %s\n", name, (long long)n, (int)probs, mask, want, totals[0],
           expect.size(), totals[1], expect_n, ok ? "ok" : "MISMATCH");
    if (!ok) {
        g_fails++;
        size_t i = 0;
        while (i < expect.size() && i < totals[0] && base[i] == (uint8_t)expect[i]) i++;
        printf("  first difference at byte %zu\n", i);
    }
    if (k <= 0) return;
    // Kraken-style lines of the same chunk: a random cut of every read's positions into segments
    std::vector<std::string> tax = {"", "5", "1234567", std::string(40, 'x')};
    std::vector<int32_t> cl, code, start;
    std::vector<u64> soff{0};
    std::string want_text;
    u64 want_lines = 0;
    for (int64_t r = 0; r < n; r++) {
        const Rec &c = ch.recs[r];
        const int64_t L = (int64_t)(off2[r + 1] - off2[r]), maxp = L - k + 1;
        const int32_t cv = (int32_t)(rng() % 5) - 1;
        cl.push_back(cv);
        std::vector<std::pair<int32_t, int32_t>> segs;
        for (int32_t p = 0; p < maxp;) {
            int32_t len = 1 + rng() % (rng() % 4 == 0 ? 2 : (rng() % 3 ? 12 : 1200));
            if (p + len > maxp) len = (int32_t)(maxp - p);
            segs.push_back({(int32_t)(rng() % 6) - 2, p});
            p += len;
        }
        for (auto &s : segs) {
            code.push_back(s.first);
            start.push_back(s.second);
        }
        soff.push_back(soff.back() + segs.size());
        if (segs.empty() || !(write_all || cv >= 0)) continue;
        want_lines++;
        want_text += cv >= 0 ? "C\t" : "U\t";
        if (c.desc.size() > 1) {
            const size_t sp = c.desc.find(' ', 1);
            want_text += c.desc.substr(1, sp == std::string::npos ? std::string::npos : sp - 1);
        }
        want_text += '\t';
        want_text += cv >= 0 ? tax[cv] : "0";
        want_text += '\t' + std::to_string(L) + '\t';
        for (size_t i = 0; i < segs.size(); i++) {
            if (i) want_text += ' ';
            const int32_t c2 = segs[i].first;
            want_text += c2 == -2 ? "A" : c2 < 0 ? "0" : tax[c2];
            want_text += ':' + std::to_string((i + 1 < segs.size() ? segs[i + 1].second : maxp) - segs[i].second);
        }
        want_text += '\n';
    }
    code.push_back(0);
    start.push_back(0);
    std::vector<uint8_t> tb;
    std::vector<uint32_t> toff{0};
    for (auto &t : tax) {
        tb.insert(tb.end(), t.begin(), t.end());
        toff.push_back((uint32_t)tb.size());
    }
    tb.push_back(0);
    std::vector<uint32_t> name_len(n + 1);
    std::vector<u64> krec(n + 1), kblocks((n + 255) / 256 + 1);
    u64 kt[2] = {0, 0};
    GsKrakenParams P{};
    P.text = (const uint8_t *)text.data();
    P.nl = nl.data();
    P.rec_line = rec_line.data();
    P.off2 = off2.data();
    P.n_reads = n;
    P.k = k;
    P.write_all = write_all;
    P.cls = cl.data();
    P.seg_off = soff.data();
    P.seg_code = code.data();
    P.seg_start = start.data();
    P.tax_bytes = tb.data();
    P.tax_off = toff.data();
    P.name_len = name_len.data();
    P.rec_out = krec.data();
    P.rec_block = kblocks.data();
    P.totals = kt;
    gs_launch_kraken_size(&P, nullptr);
    std::vector<uint8_t> kbuf(kt[0] + 64 + 16, 0xEE);
    uint8_t *kb = kbuf.data();
    while (((uintptr_t)kb & 15) != 0) kb++;
    kb += 16;
    P.out = kb;
    if (kt[0]) gs_launch_kraken_write(&P, nullptr);
    bool kok = kt[0] == want_text.size() && kt[1] == want_lines && memcmp(kb, want_text.data(), want_text.size()) == 0;
    for (int i = 1; i <= 16; i++) kok = kok && kb[-i] == 0xEE;
    for (int i = 0; i < 16; i++) kok = kok && kb[kt[0] + i] == 0xEE;
    printf("%-34s kraken k %d write_all %d: bytes %llu (want %zu) lines %llu (want %llu) %s\n", name, k, write_all, kt[0], want_text.size(), kt[1], want_lines,
           kok ? "ok" : "MISMATCH");
    if (!kok) g_fails++;
}

static Rec fasta_rec(std::mt19937_64 &rng, size_t dl, int lines, size_t width, bool crlf) {
    Rec r;
    r.desc = ">" + letters(rng, dl ? dl - 1 : 0, "abc d", 5);
    for (int i = 0; i < lines; i++) r.seq.push_back(letters(rng, i + 1 < lines ? width : 1 + rng() % width, "ACGT", 4));
    if (crlf) {
        r.desc += '\r';
        for (auto &s : r.seq) s += '\r';
    }
    return r;
}

// sequence of L bases over n_seq lines, qualities over n_qual lines, the last of them `over` characters too long
static Rec fastq_rec(std::mt19937_64 &rng, const std::string &desc, size_t L, int n_seq, int n_qual, size_t over, bool crlf) {
    Rec r;
    r.desc = desc;
    const std::string s = letters(rng, L, "ACGT", 4), q = letters(rng, L + over, "IJKL#~", 6);
    auto cut = [crlf](const std::string &x, int n, std::vector<std::string> &out, size_t extra) {
        // n lines; only the last may carry what is beyond the read's length
        const size_t body = x.size() - extra, per = std::max<size_t>(1, (body + n - 1) / n);
        size_t a = 0;
        for (int i = 0; i < n; i++) {
            size_t b = i + 1 == n ? x.size() : std::min(body > 0 ? body - 1 : 0, a + per);
            if (b < a) b = a;
            out.push_back(x.substr(a, b - a) + (crlf ? "\r" : ""));
            a = b;
        }
    };
    cut(s, n_seq, r.seq, 0);
    cut(q, n_qual, r.qual, over);
    if (crlf) r.desc += '\r';
    return r;
}

int main() {
    std::mt19937_64 rng(7);
    const std::vector<uint8_t> none;
    // FASTA: header-only records at the start, in the middle and at the end; descriptor lengths 1 .. 17
    for (int crlf = 0; crlf < 2; crlf++) {
        Chunk c;
        c.fasta = true;
        c.recs.push_back(fasta_rec(rng, 3, 0, 60, crlf));
        for (int i = 1; i <= 17; i++) c.recs.push_back(fasta_rec(rng, i, 1 + i % 3, 60, crlf));
        c.recs.push_back(fasta_rec(rng, 5, 0, 60, crlf));
        for (int i = 17; i >= 1; i--) c.recs.push_back(fasta_rec(rng, i, 1 + i % 4, 33, crlf));
        c.recs.push_back(fasta_rec(rng, 4, 0, 60, crlf));
        const int64_t n = (int64_t)c.recs.size();
        run(crlf ? "fasta crlf, all" : "fasta, all", c, none, 0, 0, false, 3, 1, rng);
        std::vector<uint8_t> f(n);
        for (auto &x : f) x = rng() % 4;
        run("fasta, mask 2 set", c, f, 2, 1, true, 31, 0, rng);
        run("fasta, clear (rest file)", c, f, 0xff, 0, false, 0, 0, rng);
        run("fasta, set (accepted file)", c, f, 0xff, 1, false, 0, 0, rng);
        std::vector<uint8_t> z(n, 0), first(n, 0), last(n, 0);
        first[0] = 1;
        last[n - 1] = 1;
        run("fasta, none", c, z, 0xff, 1, false, 0, 0, rng);
        run("fasta, first (header only)", c, first, 0xff, 1, false, 0, 0, rng);
        run("fasta, last (header only)", c, last, 0xff, 1, false, 0, 0, rng);
    }
    // general FASTQ: every shape of a record, half a record behind them
    for (int crlf = 0; crlf < 2; crlf++) {
        Chunk c;
        int id = 0;
        for (int n_seq = 1; n_seq <= 3; n_seq++)
            for (int n_qual = 1; n_qual <= 3; n_qual++)
                for (size_t over : {(size_t)0, (size_t)1, (size_t)20})
                    for (size_t L : {(size_t)7, (size_t)40, (size_t)151})
                        c.recs.push_back(fastq_rec(rng, "@r" + std::to_string(id++) + (id % 3 ? " x y" : ""), L, n_seq, n_qual, over, crlf));
        c.recs.insert(c.recs.begin() + 5, fastq_rec(rng, "@", 30, 2, 1, 0, crlf));
        if (!crlf) c.recs.insert(c.recs.begin() + 9, fastq_rec(rng, "", 30, 1, 2, 3, false));  // an empty descriptor line
        c.recs.push_back(fastq_rec(rng, "Xnot-an-at", 16, 1, 1, 0, crlf));                       // any first byte is kept
        c.tail = crlf ? "@half\r\nACGTACGT\r\nACGT\r\n+\r\nIIII\r\n" : "@half\nACGTACGT\nACGT\n+\nIIII\n";
        const int64_t n = (int64_t)c.recs.size();
        std::vector<uint8_t> f(n);
        for (auto &x : f) x = rng() % 4;
        run(crlf ? "fastq crlf, all, qualities" : "fastq, all, qualities", c, none, 0, 0, true, 3, 1, rng);
        run("fastq, all, '~'", c, none, 0, 0, false, 0, 0, rng);
        run("fastq, mask 2, qualities", c, f, 2, 1, true, 31, 0, rng);
        run("fastq, clear, qualities", c, f, 0xff, 0, true, 0, 0, rng);
        std::vector<uint8_t> z(n, 0), first(n, 0), last(n, 0);
        first[0] = 1;
        last[n - 1] = 1;
        run("fastq, none", c, z, 0xff, 1, true, 0, 0, rng);
        run("fastq, first", c, first, 0xff, 1, true, 0, 0, rng);
        run("fastq, last", c, last, 0xff, 1, true, 0, 0, rng);
    }
    // the block scan's seams
    for (int n : {1, 255, 256, 257, 513}) {
        Chunk a, b;
        a.fasta = true;
        for (int i = 0; i < n; i++) {
            a.recs.push_back(fasta_rec(rng, 1 + i % 17, i % 7 == 3 ? 0 : 1 + i % 3, 20, false));
            b.recs.push_back(fastq_rec(rng, "@q" + std::to_string(i), 5 + i % 50, 1 + i % 3, 1 + (i / 3) % 3, i % 5 == 0 ? 9 : 0, false));
        }
        std::vector<uint8_t> f(n);
        for (auto &x : f) x = rng() % 2;
        run("fasta, seams", a, f, 0xff, 1, false, 4, 1, rng);
        run("fastq, seams, qualities", b, f, 0xff, 0, true, 4, 1, rng);
    }
    // totals just below, at and just above one and two pieces; one record of more than two pieces
    for (size_t total : {(size_t)4095, (size_t)4096, (size_t)4097, (size_t)8191, (size_t)8192, (size_t)8193, (size_t)20000}) {
        Chunk a;
        a.fasta = true;
        // ">ab" + one line of L bases: 3 + 2 L + 5 bytes of text; two records, the second fills up
        const size_t first_L = 100, rest = total - (3 + 2 * first_L + 5);
        for (size_t L : {first_L, (rest - 8 - (rest & 1 ? 1 : 0)) / 2}) {
            Rec r;
            r.desc = (&L != nullptr && a.recs.size() == 1 && (rest & 1)) ? ">abc" : ">ab";
            r.seq.push_back(letters(rng, L, "ACGT", 4));
            a.recs.push_back(r);
        }
        run("fasta, piece boundary", a, none, 0, 0, false, 31, 1, rng);
        Chunk b;
        b.recs.push_back(fastq_rec(rng, "@long", total / 2, 3, 2, 5, false));
        b.recs.push_back(fastq_rec(rng, "@short", 9, 1, 1, 0, false));
        run("fastq, long record, qualities", b, none, 0, 0, true, 2, 1, rng);
    }
    printf("fails %d\n", g_fails);
    return g_fails != 0;
}
