"""Hand-worked cases of the fastasgenbank goal: what AssemblySummaryReader.getRelevantEntries over Commons CSV (quote = null, comment
marker '#', TAB, ignoreEmptyLines) makes of a text, written out -- not computed by tests/asmsum.py, which is held to these values
like everything else.  A node is an index into KNOWN.

CASES[name] = (text, cfg keywords, entries, counted, short, skipped, throws, device)
  entries  [(node, taxid, species_taxid, ftp, quality, is_ref, line)] in input order (line 0-based)
  counted  records of 20 fields and more; short: records of fewer; skipped: comment and empty lines
  throws   None, or the 1-based line of a kept entry with an empty ftp field
  device   -1 if the text, submitted as the end of a stream, lies inside the device's grammar, else the 0-based line that refuses it
"""

KNOWN = (7, 562, 9606, 10090)
FTP = b"https://ftp.ncbi.nlm.nih.gov/genomes/all/GCA/000/005/845/GCA_000005845.2_ASM584v2"


def rec(cat=b"na", taxid=b"562", species=b"562", status=b"latest", level=b"Complete Genome", ftp=FTP, n_fields=22, organism=b"Escherichia coli"):
    """one record of n_fields fields without its terminator; fields 4 5 6 7 10 11 19 as given (those that exist)"""
    f = [b"c%d" % i for i in range(n_fields)]
    for i, v in ((4, cat), (5, taxid), (6, species), (7, organism), (10, status), (11, level), (19, ftp)):
        if i < n_fields:
            f[i] = v
    return b"\t".join(f)


def E(node, taxid, species, line, quality=1, is_ref=False, ftp=FTP):
    return (node, taxid, species, ftp, quality, is_ref, line)


ALL = {"quality_mask": -1}

CASES = {
    "fields_19": (rec(n_fields=19) + b"\n", {}, [], 0, 1, 0, None, -1),
    "fields_20": (rec(n_fields=20) + b"\n", {}, [E(1, b"562", b"562", 0)], 1, 0, 0, None, -1),
    # 19 fields and a trailing tab are 20 fields, the last one empty: the key names no node here, so nothing is kept
    "tabs_19_empty_last_dropped": (rec(taxid=b"11", n_fields=19) + b"\t\n", {}, [], 1, 0, 0, None, -1),
    "tabs_19_empty_last_kept_throws": (rec(n_fields=19) + b"\t\n", {}, [], 0, 0, 0, 1, 0),
    "comments": (b"#first\n\n#after an empty line\n#after a comment\n" + rec() + b"\n", {}, [E(1, b"562", b"562", 4)], 1, 0, 4, None, -1),
    "comment_of_20_fields": (b"#" + rec() + b"\n" + rec() + b"\n", {}, [E(1, b"562", b"562", 1)], 1, 0, 1, None, -1),
    "hash_inside_a_field": (rec(cat=b"#na") + b"\n" + b"a#\t" + rec() + b"\n", {}, [E(1, b"562", b"562", 0)], 2, 0, 0, None, -1),
    "empty_lines": (b"\n\n" + rec() + b"\n\n\n", {}, [E(1, b"562", b"562", 2)], 1, 0, 4, None, -1),
    "unterminated_last_line": (rec(taxid=b"7") + b"\n" + rec(), {}, [E(0, b"7", b"562", 0), E(1, b"562", b"562", 1)], 2, 0, 0, None, -1),
    "unterminated_with_trailing_tab": (rec(taxid=b"11", n_fields=19) + b"\t", {}, [], 1, 0, 0, None, -1),
    "unterminated_short_with_trailing_tab": (rec(n_fields=18) + b"\t", {}, [], 0, 1, 0, None, -1),
    "keys_that_name_no_node": (b"".join(rec(taxid=k) + b"\n" for k in (b"", b"007", b"1234567890", b"56a", b"11", b" 562", b"0")), {}, [], 7, 0, 0, None, -1),
    "key_outside_the_filter": (rec(taxid=b"7") + b"\n" + rec(taxid=b"9606") + b"\n", {"filter": {2}}, [E(2, b"9606", b"562", 1)], 2, 0, 0, None, -1),
    "every_quality": (b"".join(rec(level=lv, status=st) + b"\n" for lv in (b"Complete Genome", b"Chromosome", b"Scaffold", b"Contig", b"Other")
                               for st in (b"latest", b"replaced")), ALL,
                      [E(1, b"562", b"562", i, quality=i + 1) for i in range(10)], 10, 0, 0, None, -1),
    "empty_level": (rec(level=b"") + b"\n" + rec(level=b"", status=b"") + b"\n", ALL,
                    [E(1, b"562", b"562", 0, quality=9), E(1, b"562", b"562", 1, quality=10)], 2, 0, 0, None, -1),
    "latest_is_exact": (rec(status=b"Latest") + b"\n" + rec(status=b"latest ") + b"\n" + rec(status=b"latest") + b"\n", ALL,
                        [E(1, b"562", b"562", 0, quality=2), E(1, b"562", b"562", 1, quality=2), E(1, b"562", b"562", 2, quality=1)], 3, 0, 0, None, -1),
    "level_is_exact": (rec(level=b"complete genome") + b"\n" + rec(level=b"Complete Genome ") + b"\n" + rec(level=b"Contigs") + b"\n", ALL,
                       [E(1, b"562", b"562", i, quality=9) for i in range(3)], 3, 0, 0, None, -1),
    "reference_against_representative": (rec(cat=b"reference genome") + b"\n" + rec(cat=b"representative genome") + b"\n" + rec(cat=b"Reference genome") + b"\n", {},
                                         [E(1, b"562", b"562", 0, is_ref=True), E(1, b"562", b"562", 1), E(1, b"562", b"562", 2)], 3, 0, 0, None, -1),
    "reference_only": (rec(cat=b"representative genome") + b"\n" + rec(cat=b"reference genome", taxid=b"7") + b"\n" + rec() + b"\n", {"reference_only": True},
                       [E(0, b"7", b"562", 1, is_ref=True)], 3, 0, 0, None, -1),
    "species_taxid_unused": (rec(taxid=b"11", species=b"9606") + b"\n", {}, [], 1, 0, 0, None, -1),
    "species_taxid_used": (rec(taxid=b"11", species=b"9606") + b"\n" + rec(taxid=b"562", species=b"12") + b"\n", {"use_species_taxid": True},
                           [E(2, b"11", b"9606", 0)], 2, 0, 0, None, -1),
    "mask_null": (rec(level=b"Contig") + b"\n" + rec(level=b"Chromosome", status=b"x") + b"\n", ALL,
                  [E(1, b"562", b"562", 0, quality=7), E(1, b"562", b"562", 1, quality=4)], 2, 0, 0, None, -1),
    "mask_empty": (rec() + b"\n" + rec(level=b"Contig") + b"\n", {"quality_mask": 0}, [], 2, 0, 0, None, -1),
    "mask_default": (rec(level=b"Chromosome") + b"\n" + rec(level=b"Chromosome", status=b"x") + b"\n" + rec(level=b"Scaffold") + b"\n" + rec(status=b"x") + b"\n" + rec() + b"\n", {},
                     [E(1, b"562", b"562", 0, quality=3), E(1, b"562", b"562", 4, quality=1)], 5, 0, 0, None, -1),
    "ftp_paths": (rec(ftp=b"https://h/a/GCA_9/") + b"\n" + rec(ftp=b"na") + b"\n" + rec(ftp=b"/") + b"\n", {},
                  [E(1, b"562", b"562", 0, ftp=b"https://h/a/GCA_9/"), E(1, b"562", b"562", 1, ftp=b"na"), E(1, b"562", b"562", 2, ftp=b"/")], 3, 0, 0, None, -1),
    "ftp_empty_throws": (b"#c\n" + rec() + b"\n" + rec(ftp=b"") + b"\n" + rec() + b"\n", {}, [], 0, 0, 0, 3, 2),
    "ftp_empty_dropped": (rec(ftp=b"", level=b"Contig") + b"\n" + rec(ftp=b"", taxid=b"5") + b"\n", {}, [], 2, 0, 0, None, -1),
    "cr_lf": (rec() + b"\r\n" + rec(taxid=b"7") + b"\r\n", {}, [E(1, b"562", b"562", 0), E(0, b"7", b"562", 1)], 2, 0, 0, None, 0),
    # a lone CR in field 7 ends the line there: 8 fields, then 15
    "lone_cr_splits_a_line": (rec() + b"\n" + rec(organism=b"Esch\rcoli") + b"\n", {}, [E(1, b"562", b"562", 0)], 1, 2, 0, None, 1),
    # ... and behind field 1 it leaves 2 fields and then 21: the second part is a record whose key is what stood in field 7
    "lone_cr_leaves_a_record": (rec(organism=b"9606")[:5] + b"\r" + rec(organism=b"9606")[6:] + b"\n", {"use_species_taxid": True},
                                [], 1, 1, 0, None, 0),
    "cr_at_the_end_of_the_stream": (rec() + b"\r", {}, [E(1, b"562", b"562", 0)], 1, 0, 0, None, 0),
    "cr_cr_lf": (rec() + b"\r\r\n" + rec() + b"\n", {}, [E(1, b"562", b"562", 0), E(1, b"562", b"562", 2)], 2, 0, 1, None, 0),
    "high_byte_in_the_organism": (rec(organism=b"Escherichia c\xc3\xb6li") + b"\n", {}, [E(1, b"562", b"562", 0)], 1, 0, 0, None, -1),
    "high_byte_in_a_short_record": (b"\xc3\xb6\t\xc3\xb6\t\xc3\xb6\t\xc3\xb6\t\xc3\xb6\t\xc3\xb6\t\xc3\xb6\n" + rec() + b"\n", {}, [E(1, b"562", b"562", 1)], 1, 1, 0, None, -1),
    "high_byte_in_the_other_taxid": (rec(species=b"56\xc3\xb6") + b"\n", {}, [E(1, b"562", b"56\xc3\xb6", 0)], 1, 0, 0, None, -1),
    # U+0131 cut to its low byte is '1': the key reads 10090
    "high_byte_in_the_key": (rec() + b"\n" + rec(taxid=b"\xc4\xb10090") + b"\n", {}, [E(1, b"562", b"562", 0), E(3, b"\xc4\xb10090", b"562", 1)], 2, 0, 0, None, 1),
    "malformed_utf8_in_the_key": (rec(taxid=b"56\xff2") + b"\n", {}, [], 1, 0, 0, None, 0),
    "nul_bytes_are_data": (rec(taxid=b"56\x002") + b"\n" + rec(organism=b"a\x00b") + b"\n", {}, [E(1, b"562", b"562", 1)], 2, 0, 0, None, -1),
}
# in the "lone_cr_leaves_a_record" case the second part starts in field 1: its field 6 is c7's neighbour -- worked out below
#   rec() = c0 c1 c2 c3 na 562 562 9606 c8 c9 latest "Complete Genome" c12 ... ; cut behind "c0\tc1" (5 bytes), the CR replaces the tab:
#   part 1: c0 c1 (2 fields, short); part 2: c2 c3 na 562 562 9606 c8 c9 latest ... c21 (20 fields): field 4 = 562, field 5 = 9606,
#   field 6 = c8 -> use_species_taxid: the key "c8" names no node; counted 1.

FILE_NAMES = [
    (FTP, b"GCA_000005845.2_ASM584v2_genomic.fna.gz"),
    (b"https://h/a/GCA_9/", b"GCA_9_genomic.fna.gz"),
    (b"na", b"na_genomic.fna.gz"),
    (b"/", b"_genomic.fna.gz"),
    (b"//", b"_genomic.fna.gz"),
    (b"a/", b"a_genomic.fna.gz"),
    (b"/a", b"a_genomic.fna.gz"),
    (b"a/b/c", b"c_genomic.fna.gz"),
]

# the cap: (qualities of one node's entries in input order, max_per_node, the entry numbers that are left, in the list's order)
CAP_CASES = [
    ([3, 1, 1], 1, [2]),        # A (3), B (1), C (1): sorted worst first A B C, cut from the front: C
    ([3, 1, 1], 2, [1, 2]),
    ([3, 1, 1], 3, [0, 1, 2]),  # count = max: not cut, input order
    ([1, 3, 1], 3, [0, 1, 2]),
    ([1, 3, 1], 5, [0, 1, 2]),  # count < max
    ([1, 3, 1], 0, [0, 1, 2]),  # max <= 0: no cap
    ([1, 3, 1], -1, [0, 1, 2]),
    ([1, 3, 1], 2, [0, 2]),     # sorted: 3 | 1 1 -> the 3 goes
    ([1, 3, 1], 1, [2]),        # ties at the cut: the later one stays
    ([1, 1, 1, 1], 2, [2, 3]),
    ([7, 1, 3, 1, 9], 3, [2, 1, 3]),  # sorted worst first: 9 7 | 3 1 1 -> order 3, then the 1s in input order
    ([2, 1], 1, [1]),
    ([1, 2], 1, [0]),
]


def cfg_of(name):
    import asmsum
    return asmsum.cfg(KNOWN, **CASES[name][1])
