"""tests/genomefasta.py -- the plain restatement of the reference's genome FASTA walk that the GPU tests compare the device with --
held to hand-written streams (tests/genomefasta_cases.py; each answer is worked out from the Java there):
  * LF, CRLF, "AC\\r\\r\\n" (all three terminators go) and "A\\rC\\n" (the '\\r' in front of a base stays);
  * an empty line inside a region gives nothing and does not end the walk (its size is 1, the loop ends at size 0);
  * a header line right behind a header line is a region of length 0;
  * data lines in front of the first header line are dropped (`first` is true, no region is open);
  * a last line without a newline keeps its bytes -- but a bare '\\r' at its end IS stripped: the while of dataLine
    (AbstractStoreFastaReader.java:95) asks for '\\n' OR '\\r', not for a '\\n' first;
  * a '>' inside a data line is a base like any other: only the first byte of a line is compared;
  * a NUL byte never reaches the line (BufferedLineReader.nextLine does not advance over it)."""
import numpy as np
import pytest

import genomefasta
from genomefasta_cases import CASES


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_gives_the_worked_answer(case):
    _, data, last, headers, seq, offsets, max_line, consumed = case
    assert genomefasta.read_fasta(data, last) == (headers, seq, offsets, max_line, consumed)


def test_the_cases_cover_what_the_issue_lists():
    names = {c[0] for c in CASES}
    for must in ("LF", "CRLF", "two CR", "CR inside a line", "empty lines", "header-only records", "data in front of the first header",
                 "no final newline", "final bare CR", "'>' inside a data line"):
        assert must in names, must


def test_next_line_and_data_line():
    assert genomefasta.next_line(b"AC\nGT", 0) == (b"AC\n", 3)
    assert genomefasta.next_line(b"AC\nGT", 3) == (b"GT", 5)
    assert genomefasta.next_line(b"AC\nGT", 5) == (b"", 5)
    assert genomefasta.next_line(b"A\x00\x00C\n", 0) == (b"AC\n", 5)
    assert genomefasta.data_line(b"AC\r\n") == b"AC" and genomefasta.data_line(b"\r\r") == b"" and genomefasta.data_line(b"\rA\r") == b"\rA"


def test_chunks_put_together_give_the_stream():
    """a stream walked in chunks -- the rest behind `consumed` in front of the next block -- gives the records of the whole stream,
    wherever the blocks end"""
    rng = np.random.default_rng(11)
    recs = []
    for i in range(12):
        body = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(rng.integers(0, 90))))
        w = int(rng.integers(1, 30))
        eol = b"\r\n" if i % 3 == 0 else b"\n"
        recs.append(b">r%d x" % i + eol + b"".join(body[j:j + w] + eol for j in range(0, len(body), w)) + (b"\n" if i % 4 == 1 else b""))
    stream = b"AA\n" + b"".join(recs)
    want = genomefasta.read_fasta(stream, True)
    for block in (1, 2, 7, 16, 33, 200, len(stream)):
        headers, parts, offsets, max_line, rest, pos = [], [], [0], 0, b"", 0
        while pos < len(stream) or rest:
            take = stream[pos:pos + block]
            pos += len(take)
            chunk, last = rest + take, pos >= len(stream)
            h, s, o, m, used = genomefasta.read_fasta(chunk, last)
            headers += h
            parts.append(s)
            offsets += [offsets[-1] + x for x in o[1:]]
            max_line = max(max_line, m)
            rest = chunk[used:]
            if last:
                break
        assert (headers, b"".join(parts), offsets) == want[:3], block
        assert max_line == want[3], block
