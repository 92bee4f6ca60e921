"""Size a genome collection on the GPU before it is built, then build it in the ranges the sizes ask for.

    python examples/size_db.py --demo

Synthetic genomes -> gs_dbsize counts (k-mers with duplicates, per species, histogram of the canonical k-mer's top bits) and
the exact number of distinct k-mers -> gs_dbsize_plan for a small memory grant -> gs_dbbuild range by range; the concatenation
of the ranges' results is the one-shot build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import genestrip_amd as ga  # noqa: E402
from genestrip_amd import synth  # noqa: E402


def demo():
    k = 31
    db = synth.SynthDB(k=k, genera=3, species_per_genus=4, genome_len=20000, seed=5, build=False)
    g = db.genomes
    seq = np.ascontiguousarray(g).reshape(-1)
    off = (np.arange(g.shape[0] + 1, dtype=np.uint64) * np.uint64(g.shape[1]))
    tags = np.asarray(db.species_vi, np.int32)

    sizer = ga.DeviceDbSizer(k, db.n_values, hist_bits=10, radix_bits=16, keep_keys=True)
    sizer.add(seq, off, tags)
    t, per_value, hist = sizer.counts()
    n_distinct, buckets = sizer.distinct()
    st = sizer.stats()
    sizer.close()
    print(f"{g.shape[0]} genomes, {seq.size} bases: {t.total} k-mers, {t.dust} dropped by the dust gate, {t.included} included")
    print(f"per species: {per_value[tags].tolist()}")
    print(f"{n_distinct} distinct k-mers, largest of {len(buckets)} radix buckets holds {int(buckets.max())}; "
          f"{st.bytes_peak / max(st.n_keys, 1):.1f} bytes per retained key at the peak")

    grant = 40 * (t.included // 4)  # bytes of device memory for the builder's pairs: a quarter of what one pass would take
    ranges = ga.plan_ranges(hist, 10, k, grant // 40)
    print(f"a grant of {grant} bytes (40 per pair) -> {len(ranges)} ranges")

    def build(lo=None, hi=None):
        b = ga.DeviceDbBuilder(k, db.n_values, db.parent_vi)
        if lo is not None:
            b.set_range(lo, hi)
        b.add(seq, off, tags)
        out = b.finish()
        b.close()
        return out

    whole = build()
    parts = [build(lo, hi) for lo, hi in ranges]
    for (lo, hi), p in zip(ranges, parts):
        print(f"  [{lo:#018x}, {hi:#018x}): {len(p[0])} k-mers")
    same = np.array_equal(np.concatenate([p[0] for p in parts]), whole[0]) and np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    assert same and len(whole[0]) == n_distinct
    print(f"the concatenation of the {len(ranges)} ranges equals the one-shot build: {len(whole[0])} k-mers")


if __name__ == "__main__":
    if "--demo" not in sys.argv[1:]:
        sys.exit(__doc__)
    demo()
