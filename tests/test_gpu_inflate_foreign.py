"""The device DEFLATE decoders (gs_inflate_members: BGZF, one wave per member; gs_gunzip_device: single-member gzip in segments) on
streams zlib never writes -- tests/inflate_cases.py, written by tests/deflatewriter.py, every one accepted (or rejected) by zlib in
tests/test_inflate_cases_cpu.py.  A legal stream must come out byte for byte on both paths; a refusal to the host decoders (GsError -4 /
-2) is a failure here: these streams fit one batch, so no documented capacity refusal applies to them, and a decoder that wrongly rejects
a legal stream would otherwise only make the file slower, unnoticed.  A damaged stream must be reported.  Run with -m gpu."""
import pytest

import deflatewriter as dw
import genestrip_amd as ga
import inflate_cases as ic

pytestmark = pytest.mark.gpu

BGZF_GROUPS = sorted(g for g, cases in ic.groups().items() if any(not c.gzip_only for c in cases))
GZIP_GROUPS = sorted(ic.groups())


def _inflate_group(cases):
    """the members of a group in one buffer and one call: every status 0, every member's bytes its text"""
    data = b"".join(dw.bgzf_member(c.payload, c.text) for c in cases)
    members, reached = ga.bgzf_members(data)
    assert reached == len(data) and len(members) == len(cases)
    try:
        got, st = ga.inflate_members(data, members)
    except ga.GsError as e:
        pytest.fail("inflate_members: %s; status %s" % (e, {c.name: int(s) for c, s in zip(cases, e.status) if s}))
    assert not st.any()
    got, at = got.tobytes(), 0
    for c in cases:
        part = got[at:at + len(c.text)]
        if part != c.text:
            first = next(i for i in range(len(c.text)) if part[i] != c.text[i])
            pytest.fail("%s: text differs from byte %d of %d on" % (c.name, first, len(c.text)))
        at += len(c.text)


@pytest.mark.parametrize("group", BGZF_GROUPS)
def test_foreign_streams_as_bgzf_members(group):
    _inflate_group([c for c in ic.groups()[group] if not c.gzip_only])


@pytest.mark.parametrize("group", ["random_codes", "deep48", "one_dist_code"])
def test_foreign_streams_through_the_canonical_decoder(monkeypatch, group):
    """the table-free decoder, which no stream reaches on its own, on the codes that are hardest on it: 15-bit codes, a lone distance code"""
    monkeypatch.setenv("GS_INFLATE_FORCE_SLOW", "1")
    _inflate_group(ic.groups()[group])


@pytest.mark.parametrize("chunk", ["4096", None])
@pytest.mark.parametrize("group", GZIP_GROUPS)
def test_foreign_streams_as_single_member_gzip(monkeypatch, group, chunk):
    """many segments (chunks of 4 KiB) and the default chunk; no refusal counts as a pass"""
    if chunk:
        monkeypatch.setenv("GS_GUNZIP_CHUNK", chunk)
    for c in ic.groups()[group]:
        # (the inner stream's block starts are text and pass the finder's test either way; its own bytes are not text)
        for any_bytes in ("0", "1") if group == "nested_gzip" else ("1",) if c.any_bytes else (None,):
            if any_bytes is not None:
                monkeypatch.setenv("GS_GUNZIP_ANY_BYTES", any_bytes)
            else:
                monkeypatch.delenv("GS_GUNZIP_ANY_BYTES", raising=False)
            try:
                got, info = ga.gunzip_device(dw.gzip_member(c.payload, c.text), len(c.text))
            except ga.GsError as e:
                pytest.fail("%s (chunk %s, any bytes %s): %s" % (c.name, chunk, any_bytes, e))
            assert got.tobytes() == c.text, (c.name, chunk, any_bytes)
            if group == "nested_gzip":  # (every block start of the inner file, found inside the outer one's stored blocks, is a false one)
                assert info[3] >= 10, info


def test_false_block_starts_in_many_batches(monkeypatch):
    """the gzip file inside another in batches of four chunks: a batch's last segment runs past the false starts found behind the batch
    and the batch ends at the boundary it stopped at, the next one starts there"""
    monkeypatch.setenv("GS_GUNZIP_SLOTS", "4")
    monkeypatch.setenv("GS_GUNZIP_CHUNK", "4096")
    for c in ic.groups()["nested_gzip"]:
        for upload in ("whole", "per_batch"):
            if upload == "per_batch":
                monkeypatch.setenv("GS_GUNZIP_WHOLE_MAX", "0")
            try:
                got, info = ga.gunzip_device(dw.gzip_member(c.payload, c.text), len(c.text))
            except ga.GsError as e:
                pytest.fail("%s (%s): %s" % (c.name, upload, e))
            assert got.tobytes() == c.text, (c.name, upload)
            assert info[2] >= 5 and info[3] >= 10, info


def test_damaged_foreign_streams_are_reported():
    """every stream of the `rejected` group between two good members: its status is non-zero, the good ones come out all the same;
    the single-member path raises and never returns text"""
    good = ic.groups()["alt258"][0]
    for c in ic.rejected():
        data = dw.bgzf_member(good.payload, good.text) + dw.bgzf_member(c.payload, c.text) + dw.bgzf_member(good.payload, good.text)
        members, reached = ga.bgzf_members(data)
        assert reached == len(data) and len(members) == 3
        with pytest.raises(ga.GsError) as e:
            ga.inflate_members(data, members)
        assert e.value.code == -1 and list(e.value.status != 0) == [False, True, False], (c.name, e.value.status)
        with pytest.raises(ga.GsError):
            ga.gunzip_device(dw.gzip_member(c.payload, c.text), len(c.text) + 4096)
