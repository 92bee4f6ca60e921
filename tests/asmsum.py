"""The fastasgenbank goal restated in plain Python: the records of an assembly summary as Commons CSV 1.9.0 cuts them (quote = null,
comment marker '#', delimiter TAB, ignoreEmptyLines, no escape, no trimming, UTF-8), AssemblySummaryReader.getRelevantEntries
(C/genbank/AssemblySummaryReader.java:104-144), AssemblyEntry's file name (:170-192), AssemblyQuality.fromString (:294-308), the
node of a tax id string (C/tax/TaxTree.java:367-369 over C/util/DigitTrie.java:192-225) and the cap of FastaFilesFromGenbankGoal
(C/goals/genbank/FastaFilesFromGenbankGoal.java:101-150).  The tests hold the host parser, the handles and the file loop to this
file; tests/asmsum_cases.py holds this file to values worked out by hand."""
import random
import re

QUALITIES = ("ADDITIONAL", "COMPLETE_LATEST", "COMPLETE", "CHROMOSOME_LATEST", "CHROMOSOME", "SCAFFOLD_LATEST", "SCAFFOLD",
             "CONTIG_LATEST", "CONTIG", "LATEST", "NONE")
LEVELS = {b"Complete Genome": 1, b"Chromosome": 3, b"Scaffold": 5, b"Contig": 7}
DEFAULT_MASK = 1 << 1 | 1 << 3
MAX_LINE = 4096  # GS_AS_MAX_LINE: the longest line, its newline included, that the device takes


class EmptyFtp(Exception):
    """a kept entry has an empty ftp field: the reference throws; .line is 1-based"""

    def __init__(self, line):
        super().__init__(f"line {line}")
        self.line = line


def cfg(known, filter=None, quality_mask=DEFAULT_MASK, reference_only=False, use_species_taxid=False):
    """known: ascending tax ids, a node is an index; filter: a set of nodes or None; quality_mask: bit q allows ordinal q, -1 all"""
    return {"known": list(known), "filter": None if filter is None else set(filter), "quality_mask": quality_mask,
            "reference_only": reference_only, "use_species_taxid": use_species_taxid}


def lines_of(text):
    """every line of the stream without its terminator: LF, CR or CR LF ends one; an unterminated last line counts"""
    out = re.split(b"\r\n|\r|\n", bytes(text))
    if out[-1] == b"":
        out.pop()
    return out


def quality_of(level, status):
    latest = status == b"latest"
    q = LEVELS.get(bytes(level))
    return (q if latest else q + 1) if q is not None else (9 if latest else 10)


def low_bytes(key):
    """the UTF-16 units of the decoded key, each cut to its low byte"""
    units = bytes(key).decode("utf-8", errors="replace").encode("utf-16-le")
    return bytes(units[0::2])


def node_of(key, known):
    s = low_bytes(key)
    if not s or not s.isdigit() or not all(0x30 <= c <= 0x39 for c in s) or s[0] == 0x30 or len(s) > 10:
        return -1
    v = int(s)
    lo, hi = 0, len(known)
    while lo < hi:
        mid = (lo + hi) // 2
        if known[mid] < v:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < len(known) and known[lo] == v else -1


def file_name_of(ftp):
    ftp = bytes(ftp)
    pos = ftp.rfind(b"/")
    if pos == len(ftp) - 1:
        if not ftp:
            raise ValueError("empty ftp path")
        prev = ftp.rfind(b"/", 0, pos)
        base = ftp[prev + 1:pos]
    else:
        base = ftp[pos + 1:]
    return base + b"_genomic.fna.gz"


def judge(fields, c):
    """a counted record -> None (dropped), or (node, quality, is_ref); an empty ftp field of a kept one is the caller's to raise"""
    node = node_of(fields[6] if c["use_species_taxid"] else fields[5], c["known"])
    if node < 0 or (c["filter"] is not None and node not in c["filter"]):
        return None
    q = quality_of(fields[11], fields[10])
    if not (c["quality_mask"] >> q & 1):
        return None
    is_ref = fields[4] == b"reference genome"
    if c["reference_only"] and not is_ref:
        return None
    return node, q, is_ref


def relevant_entries(text, c, first_line=0):
    """-> (entries in input order, counted, short records, comment and empty lines); an entry is
    (node, taxid, species_taxid, ftp, quality, is_ref, line)"""
    entries, counted, short, skipped = [], 0, 0, 0
    for no, ln in enumerate(lines_of(text)):
        if not ln or ln[:1] == b"#":
            skipped += 1
            continue
        f = ln.split(b"\t")
        if len(f) < 20:
            short += 1
            continue
        counted += 1
        got = judge(f, c)
        if got is None:
            continue
        if not f[19]:
            raise EmptyFtp(first_line + no + 1)
        entries.append((got[0], f[5], f[6], f[19], got[1], got[2], first_line + no))
    return entries, counted, short, skipped


def cap(entries, max_per_node):
    """-> the picked entries: nodes ascending, inside a node the reference's list order"""
    by_node = {}
    for e in entries:
        by_node.setdefault(e[0], []).append(e)
    out = []
    for node in sorted(by_node):
        lst = by_node[node]
        if max_per_node > 0 and len(lst) > max_per_node:
            lst = sorted(lst, key=lambda e: -e[4])  # (stable) lowest quality first
            lst = lst[len(lst) - max_per_node:]
        out.extend(lst)
    return out


def in_grammar(chunk, c, last=False):
    """-> -1 if the device takes the chunk, else the 0-based line that refuses it (the first)"""
    chunk = bytes(chunk)
    if not chunk:
        return -1
    lines = chunk.split(b"\n")
    terminated = lines[-1] == b""
    if terminated:
        lines.pop()
    for no, ln in enumerate(lines):
        tail = no == len(lines) - 1 and not terminated
        if b"\r" in ln or len(ln) + (0 if tail else 1) > MAX_LINE or (tail and not last):
            return no
        if not ln or ln[:1] == b"#":
            continue
        f = ln.split(b"\t")
        if len(f) < 20:
            continue
        if any(b >= 0x80 for b in (f[6] if c["use_species_taxid"] else f[5])):
            return no
        if judge(f, c) is not None and not f[19]:
            return no
    return -1


# ---- generated summaries of NCBI's column layout (38 columns)
SUBMITTERS = ["Institut für Mikrobiologie", "Université de Montréal", "DOE Joint Genome Institute", "北京大学", "Broad Institute"]
LEVEL_NAMES = ["Complete Genome", "Chromosome", "Scaffold", "Contig", "Contig", "Scaffold", "complete genome"]


def summary_line(rng, known, i):
    taxid = rng.choice(known) if rng.random() < 0.8 else rng.randrange(1, 3_000_000)
    species = rng.choice(known) if rng.random() < 0.8 else taxid
    acc = f"GCA_{i:09d}.{rng.randrange(1, 4)}"
    asm = f"ASM{rng.randrange(1000, 999999)}v{rng.randrange(1, 3)}"
    cat = rng.choice(["reference genome", "representative genome", "na", "na", "na"])
    status = rng.choice(["latest", "latest", "latest", "replaced", "suppressed"])
    level = rng.choice(LEVEL_NAMES)
    ftp = rng.choice([f"https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA/{i // 1000000 % 1000:03d}/{i // 1000 % 1000:03d}/{i % 1000:03d}/{acc}_{asm}",
                      f"https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA/000/000/{i % 1000:03d}/{acc}_{asm}/", "na"])
    f = [acc, f"PRJNA{rng.randrange(1, 999999)}", f"SAMN{rng.randrange(1, 99999999):08d}", "", cat, str(taxid), str(species),
         "Escherichia coli str. " + "x" * rng.randrange(0, 40), "strain=K-12", "", status, level, "Major", "Full", "2020/01/0%d" % rng.randrange(1, 10), asm,
         rng.choice(SUBMITTERS), "na", "", ftp, "", "na", "assembly from type material" if rng.random() < 0.1 else "na", "haploid", "bacteria",
         str(rng.randrange(100000, 9999999)), str(rng.randrange(100000, 9999999)), "50.5", "1", "1", str(rng.randrange(1, 300)), "NCBI RefSeq", "2020/01/01",
         "1000", "900", "80", "na", "na"]
    assert len(f) == 38
    return "\t".join(f)


def summary(n_lines, known, seed=1, header=True):
    """-> bytes: n_lines records in NCBI's layout behind its two comment lines, with non-ASCII submitter names, a few short records
    and a few empty lines"""
    rng = random.Random(seed)
    out = ["## See ftp://ftp.ncbi.nlm.nih.gov/genomes/README_assembly_summary.txt for a description of the columns in this file.",
           "#assembly_accession\tbioproject\tbiosample"] if header else []
    for i in range(n_lines):
        r = rng.random()
        if r < 0.01:
            out.append("")
        elif r < 0.02:
            out.append("\t".join(summary_line(rng, known, i).split("\t")[:rng.randrange(1, 20)]))
        else:
            out.append(summary_line(rng, known, i))
    return ("\n".join(out) + "\n").encode("utf-8")
