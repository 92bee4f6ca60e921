"""The reference's walk over a genome FASTA stream, restated line by line in plain Python.  A helper module of the suite, not a
test file, and independent of the library: nothing here calls it.  tests/test_genomefasta_cpu.py pins it on hand-written cases.

Three functions of the reference are restated (paths relative to the reference's source tree):
  BufferedLineReader.nextLine       base/.../io/BufferedLineReader.java:160-182     -> next_line
  AbstractFastaReader.readFasta     core/.../fasta/AbstractFastaReader.java:97-130   -> the loop of read_fasta
  AbstractStoreFastaReader.dataLine core/.../refseq/AbstractStoreFastaReader.java:87-114 -> data_line
with every region included (which regions count is decided behind this parse, from the header lines)."""

NL, CR, GT = 10, 13, 62


def next_line(data, pos):
    """-> (line, next pos): the bytes up to and including the next '\\n' (or up to the end of the stream), NUL bytes dropped
    (nextLine copies a byte and advances `size` only if it is not 0, :168-171); an empty line at the end of the stream: size 0"""
    end = data.find(b"\n", pos)
    end = len(data) if end < 0 else end + 1
    line = data[pos:end]
    if 0 in line:
        line = line.replace(b"\x00", b"")
    return line, end


def data_line(line):
    """the bases of a data line: `end` steps back over every trailing '\\n' and '\\r' (the while at :95), the bytes in front of
    it are put into the ring buffer one by one -- a '\\r' between them included"""
    end = len(line)
    while end > 0 and line[end - 1] in (NL, CR):
        end -= 1
    return line[:end]


def cut(data, last):
    """the bytes covered by the records that END inside the chunk: all of it if the stream ends here; else up to the start of the
    last header line (a later header line is what ends a record); without any header line up to behind the last newline (whole
    lines that belong to no region, or to one whose header the caller has seen in an earlier chunk)"""
    if last:
        return len(data)
    pos = data.rfind(b"\n>")
    if pos >= 0:
        return pos + 1
    if data[:1] == b">":
        return 0
    return data.rfind(b"\n") + 1


def read_fasta(data, last=True):
    """-> (headers, seq, offsets, max_line, consumed).  headers: per record its header line from '>' up to but excluding the
    '\\n'; seq / offsets: the bases of all records back to back and len(headers) + 1 offsets from 0; max_line: the largest `size`
    readFasta sees (the line with its newline; it throws from fastaLineSizeBytes - 1 on, :104); consumed: cut(data, last)"""
    data = bytes(data)
    consumed = cut(data, last)
    data = data[:consumed]
    headers, parts, offsets = [], [], [0]
    max_line, pos, total = 0, 0, 0
    first = True  # readFasta's flag: no region has been started yet, data lines are dropped
    while True:
        line, pos = next_line(data, pos)
        size = len(line)
        if size == 0:  # the for loop of readFasta ends here; only the end of the stream gives it: a line holds at least its '\n'
            break
        max_line = max(max_line, size)
        if size > 0 and line[0] == GT:
            if not first:
                offsets.append(total)  # endRegion
            first = False
            headers.append(line[:-1] if line[-1] == NL else line)
        elif not first:
            bases = data_line(line)
            parts.append(bases)
            total += len(bases)
    if not first:
        offsets.append(total)
    return headers, b"".join(parts), offsets, max_line, consumed
