// The line-by-line krakencount parser of the host layer (genestrip_amd/csrc/gs_krakenparse.h) on its own under AddressSanitizer /
// UBSan: the inputs on which the reference throws, the oddities it keeps (NUL bytes, an unterminated tail, an empty line, a
// descriptor with ':' and blanks, tokens without a class), long lines and every split of a text into two feeds.  Expected values
// are worked out by hand from KrakenResultProcessor.java:74-179 and KrakenResCountGoal.java:133-157.
#include <cstdio>
#include <string>

#include "../../genestrip_amd/csrc/gs_krakenparse.h"

using gs_host::KrakenExact;

static int fails = 0;
#define CHECK(c)                                               \
    do {                                                       \
        if (!(c)) {                                            \
            fails++;                                           \
            printf("FAILED line %d: %s\n", __LINE__, #c);      \
        }                                                      \
    } while (0)

static bool feed(KrakenExact &k, const std::string &s, bool last = true) {
    // (a copy of exactly the bytes, so that a read past either end is a heap overflow the sanitizer sees)
    std::vector<uint8_t> b(s.begin(), s.end());
    return k.feed(b.data(), b.size(), last);
}

static std::string line(const std::string &tokens, const std::string &cls = "9", const std::string &desc = "d", const std::string &size = "100") {
    return "C\t" + desc + "\t" + cls + "\t" + size + "\t" + tokens + "\n";
}

int main() {
    {  // the golden line
        KrakenExact k;
        CHECK(feed(k, "C\ttest\t1\t41\t0:2 1:7 0:2\n"));
        CHECK(k.rows.size() == 2 && k.rows["0"].kmers == 4 && k.rows["0"].reads == 0 && k.rows["1"].kmers == 7 && k.rows["1"].reads == 1 && k.rows["1"].kimr == 0);
        CHECK(k.lines == 1 && k.counted == 3 && k.a_tokens == 0 && k.ended);
    }
    // where the reference throws: the line is reported, 1-based
    const struct {
        std::string text;
        int64_t line;
    } errors[] = {{line("9:5") + line("9:5x 3:1"), 2}, {line("9:5", "9", "d", "1x0"), 1}, {line("9:5") + line("9:5") + line("9:5", "9a"), 3},
                  {"C\td\t9\t100\t9:5\r\n", 1},      {line("9:5  3:1"), 1},              {line("0:1", "7", "d1:5 22:7 z"), 1},
                  {line("9:5", "9", "d:x y"), 1},    {"x\ty:3 4:2 \n", 1},               {line("9:5") + "\t\t\t\t:\t:x \n", 2}};
    for (const auto &e : errors) {
        KrakenExact k;
        CHECK(!feed(k, e.text));
        CHECK(k.line_no == e.line && !k.error.empty());
    }
    {  // a tax id with a non-digit is skipped, 'A' tokens too; an empty class and an empty tax id are keys
        KrakenExact k;
        CHECK(feed(k, line("9x:5 A:1 9:2") + line("7:5 :3", "") + line("", "5") + line("A:1 A:2", "0")));
        CHECK(k.rows["9"].reads == 1 && k.rows["9"].kmers == 2 && k.rows["9"].kimr == 2);
        CHECK(k.rows[""].reads == 1 && k.rows[""].kmers == 3 && k.rows[""].kimr == 0 && k.rows["7"].kmers == 5);
        CHECK(k.rows.size() == 3 && k.a_tokens == 3 && k.counted == 3 && k.lines == 4);
    }
    {  // a token in front of the class field counts under the class of the line before; filtered: no class, no failure
        KrakenExact k;
        CHECK(feed(k, line("9:5", "5") + line("0:1", "7", "d1:5 22:7 z")));
        CHECK(k.rows["5"].reads == 2 && k.rows["22"].kmers == 7 && k.rows["0"].kmers == 1 && k.rows.count("7") == 0);
        KrakenExact f;
        f.filtered = true;
        CHECK(feed(f, line("0:1", "7", "d1:5 22:7 z")) && f.rows["22"].kmers == 7 && f.rows.count("7") == 0);
    }
    {  // the stream ends at an empty line; an unterminated tail loses a byte; a one-byte tail ends the stream; NUL bytes go
        KrakenExact k;
        CHECK(feed(k, line("9:5") + "\n" + line("9:7")) && k.rows["9"].kmers == 5 && k.lines == 1 && k.line_no == 2);
        KrakenExact t;
        CHECK(feed(t, line("9:5") + "C\td\t9\t100\t9:73") && t.rows["9"].kmers == 12 && t.rows["9"].reads == 2);
        KrakenExact o;
        CHECK(feed(o, line("9:5") + "x") && o.lines == 1 && o.rows["9"].kmers == 5);
        KrakenExact z;
        CHECK(feed(z, std::string("C\td\t9\t100\t9:") + '\0' + "5\n" + '\0' + "\n" + line("9:1")) && z.rows["9"].kmers == 5 && z.lines == 1);
        KrakenExact e;
        CHECK(feed(e, "") && e.ended && e.rows.empty());
    }
    {  // numbers are Java ints: 4294967297 is 1, 2147483648 is negative
        KrakenExact k;
        CHECK(feed(k, line("9:4294967297 3:2147483648")) && k.rows["9"].kmers == 1 && k.rows["3"].kmers == -2147483648LL);
    }
    {  // long lines count and are reported: 65 536 bytes with the newline is the last one the reference takes
        for (size_t n : {(size_t)65536, (size_t)65537, (size_t)300000}) {
            const std::string head = "C\t", tail = "\t9\t100\t9:5\n";
            KrakenExact k;
            CHECK(feed(k, head + std::string(n - head.size() - tail.size(), 'x') + tail));
            CHECK(k.rows["9"].kmers == 5 && k.long_lines == (n > 65536 ? 1 : 0));
        }
    }
    {  // every split of a text into two feeds of whole lines gives what one feed gives; the class lives across the feeds
        const std::string text = line("9:5 3:1", "3") + "x\ty:3 4:2 \n" + line("A:1") + line("8:1 8:2", "8") + "C\td\t9\t100\t9:73";
        KrakenExact whole;
        CHECK(feed(whole, text));
        for (size_t cut = 0; cut <= text.size(); cut++) {
            if (cut > 0 && text[cut - 1] != '\n') continue;
            KrakenExact k;
            CHECK(feed(k, text.substr(0, cut), false) && feed(k, text.substr(cut), true));
            CHECK(k.rows.size() == whole.rows.size() && k.lines == whole.lines && k.counted == whole.counted && k.line_no == whole.line_no);
            for (const auto &kv : whole.rows) {
                const auto it = k.rows.find(kv.first);
                CHECK(it != k.rows.end() && it->second.reads == kv.second.reads && it->second.kmers == kv.second.kmers && it->second.kimr == kv.second.kimr);
            }
        }
        CHECK(whole.rows["3"].reads == 2 && whole.rows["9"].kmers == 12);
        KrakenExact k;  // a class noted from a line counted elsewhere
        const std::string dev = line("1:1", "42");
        k.set_class_of((const uint8_t *)dev.data(), dev.size() - 1);
        CHECK(feed(k, "x\ty:3 4:2 \n") && k.rows["42"].reads == 1);
        k.forget_class();
        k.ended = false;
        CHECK(!feed(k, "x\ty:3 4:2 \n"));
    }
    printf("fails %d\n", fails);
    return fails != 0;
}
