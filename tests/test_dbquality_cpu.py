"""The dbquality goal without a GPU: the host layer's CSV writer (gs_host_write_quality_csv: the rank aggregation of
DBQualityCountsGoal.doMakeThis :149-173 + DBQualityCSVGoal.makeFile) against the plain-Python restatement and a hand-computed
golden file, and the CPU reference of the counts (tests/qualitycheck.py) on the dengue1 fixture's known answer."""
import json
import os

import numpy as np

import qualitycheck as qc
from conftest import GOLDEN
from genestrip_amd import host
from oracle import gs_oracle as orc

# value:     0        1        2          3         4          5         6         7          8     9        10
RANKS = ["no rank", "genus", "species", "strain", "species", "strain", "strain", "no rank", None, "genus", "species"]
PARENT = [-1, 0, 1, 2, 1, 4, 4, 0, -2, 0, 9]
TAXIDS = ["1", "100", "110", "111", "120", "121", "122", "7", "8", "200", "210"]
NAMES = ["root", "Genus one", "Species 1a", "Strain 1a1", "Species 1b", "Strain 1b1", "Strain 1b2", "Odd one", None, "Genus two",
         "Species 2a"]


def _case():
    """genus 1 has no row: species 2 (own row), strain 3, strains 5 and 6 are aggregated into it; species 2 is not aggregated into
    itself; species 4 has no row: strains 5 and 6 are aggregated into it; node 7 has no ancestor of any asked rank; genus 9 and
    species 10 have rows of their own: nothing is aggregated into either"""
    counts = np.zeros((len(PARENT), 3), np.int64)
    present = np.zeros(len(PARENT), np.uint8)
    for v, row in {2: (1, 3, 2), 3: (5, 7, 6), 5: (2, 3, 9), 6: (10, 11, 13), 7: (0, 5, 4), 9: (40, 41, 40), 10: (6, 47, 7)}.items():
        counts[v] = row
        present[v] = 1
    return counts, present


def test_quality_csv_equals_the_restatement(tmp_path):
    counts, present = _case()
    for position in (None, [0, 5, 8, 9, 6, 7, 10, 1, 99, 2, 3]):  # pre-order, and an order that puts genus two first
        want = qc.quality_csv(PARENT, TAXIDS, counts, present, NAMES, RANKS, position)
        path = tmp_path / "q.csv"
        host.write_quality_csv(path, PARENT, TAXIDS, counts, present, names=NAMES, ranks=RANKS, position=position)
        got = path.read_bytes()
        assert got == want, (got.decode(), want.decode())
    rows = {l.split(";")[0]: l.split(";") for l in want.decode().split("\n")[1:-1]}
    assert set(rows) == {"100", "110", "111", "120", "121", "122", "7", "200", "210"}
    assert rows["100"][4:7] == ["18", "24", "30"] and rows["120"][4:7] == ["12", "14", "22"]  # genus one: 4 children, species 1b: 2
    assert rows["110"][4:7] == ["1", "3", "2"] and rows["200"][4:7] == ["40", "41", "40"]      # own rows stay as they are
    assert rows["110"][7] == "0.33333333" and rows["111"][7] == "0.71428571"                    # non-terminating decimals
    # the columns NAMED precision / recall are the unweighted averages, the weighted avg columns the ratio of the sums
    assert rows["100"][7] == format((1 / 3 + 5 / 7 + 2 / 3 + 10 / 11) / 4, ".8f") and rows["100"][9] == format(18 / 24, ".8f")
    assert rows["100"][7] != rows["100"][9]
    assert rows["7"][7] == "0.00000000" and rows["7"][3] == "1"
    # the root has no row here; with one, its parent prints as null
    present[0], counts[0] = 1, (3, 4, 5)
    path = tmp_path / "r.csv"
    host.write_quality_csv(path, PARENT, TAXIDS, counts, present, names=NAMES, ranks=RANKS)
    assert path.read_bytes() == qc.quality_csv(PARENT, TAXIDS, counts, present, NAMES, RANKS)
    assert path.read_text().split("\n")[1] == "1;root;no rank;null;3;4;5;0.75000000;0.60000000;0.75000000;0.60000000;"
    # no ranks, no names: no aggregation, names print as null
    host.write_quality_csv(path, PARENT, TAXIDS, counts, present)
    assert path.read_bytes() == qc.quality_csv(PARENT, TAXIDS, counts, present)


def test_quality_csv_hand_computed_golden(tmp_path):
    g = json.load(open(os.path.join(GOLDEN, "quality_csv", "small.json")))
    want = open(os.path.join(GOLDEN, "quality_csv", "small.csv"), "rb").read()
    path = tmp_path / "g.csv"
    host.write_quality_csv(path, g["parent_vi"], g["taxids"], np.array(g["counts"], np.int64), np.array(g["present"], np.uint8),
                           names=g["names"], ranks=g["ranks"])
    assert path.read_bytes() == want
    assert qc.quality_csv(g["parent_vi"], g["taxids"], g["counts"], g["present"], g["names"], g["ranks"]) == want


def test_helper_known_answer_on_dengue1():
    """the dengue1 FASTA has 10 705 distinct canonical 31-mers; stored under one value, every one of them
    is a true positive of that leaf"""
    raw = open(os.path.join(GOLDEN, "dengue1", "dengue1.fasta"), "rb").read()
    rd = orc.parse_fastq(raw, fasta=True, k=31)
    seq = bytes(rd["seq"])
    off = rd["seq_off"].astype(np.int64)
    regions = [(seq[off[i]:off[i + 1]], 1) for i in range(len(off) - 1)]
    kmers = np.unique(np.concatenate([orc.canonical_kmers(s.decode().upper(), 31) for s, _ in regions]))
    assert len(kmers) == 10705
    parent = np.array([-1, 0], np.int32)
    ref = qc.reference_counts(31, kmers, np.ones(len(kmers), np.int32), parent, regions)
    assert ref["counts"].tolist() == [[0, 0, 0], [10705, 10705, 10705]] and ref["present"].tolist() == [0, 1]
    csv = qc.quality_csv(parent, ["1", "11053"], ref["counts"], ref["present"], ["root", "Dengue virus 1"], ["no rank", "no rank"])
    assert csv.decode().split("\n")[1] == "11053;Dengue virus 1;no rank;1;10705;10705;10705;1.00000000;1.00000000;1.00000000;1.00000000;"
