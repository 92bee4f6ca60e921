"""The extract and the fasta2fastq goal restated from the reference's Java, independent of the library: what the tests of both
goals compare against.

fasta2fastq: AbstractFastaReader.readFasta (C/fasta/AbstractFastaReader.java:97-130) with the FastqWriter of
Fasta2FastqGoal.java:118-165 over BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182).
extract: ExtractGoal.java:92-96 over AbstractFastqReader.doReadFastq / doReadFasta (:288-438) and ReadEntry.write (:570-584),
for input whose records are whole (what the goal is run on)."""

TARGET = 65535  # FastqWriter's line buffer (Fasta2FastqGoal.java:95)


class LineTooLong(Exception):
    """readFasta throws IllegalStateException("buffer is too small for data line in fasta file")"""


def next_lines(data):
    """BufferedLineReader.nextLine until it returns 0: the lines with their '\\n', NUL bytes dropped"""
    for raw in _split(bytes(data)):
        line = raw.replace(b"\0", b"")
        if not line:  # (only NUL bytes in front of the end of the stream)
            return
        yield line


def _split(data):
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl + 1
        yield data[pos:end]
        pos = end


def java_print(b):
    """PrintStream.print((char) b) per byte, UTF-8: a byte >= 0x80 is sign-extended to the char 0xFF80 .. 0xFFFF"""
    out = bytearray()
    for x in b:
        if x < 0x80:
            out.append(x)
        else:
            out += chr(0xFF00 | x).encode("utf-8")
    return bytes(out)


def fasta2fastq(data):
    """-> (the bytes the goal writes for one input stream, header lines seen)"""
    out = bytearray()
    first, data_size, records = True, 0, 0

    def end_region():
        out.extend(b"\n+\n" + b"~" * data_size + b"\n")

    for line in next_lines(data):
        size = len(line)
        if size >= TARGET - 1:
            raise LineTooLong()
        if line[0:1] == b">":
            if not first:
                end_region()
            first = False
            data_size = 0  # startRegion
            records += 1
            out.extend(b"@" + java_print(line[1:size - 1]) + b"\n")  # infoLine: println(target, 1, size - 1)
        else:
            end = size
            while end > 0 and line[end - 1:end] in (b"\n", b"\r"):
                end -= 1
            out.extend(java_print(line[:end]))
            data_size += end
    if not first:
        end_region()
    return bytes(out), records


def fasta2fastq_files(datas):
    """the goal's loop over its resources: one output"""
    return b"".join(fasta2fastq(d)[0] for d in datas)


def read_entries(data, fasta):
    """(descriptor, read, quality or None) per record, as doReadFastq / doReadFasta fill a ReadEntry"""
    lines = [ln[:-1] if ln.endswith(b"\n") else ln for ln in next_lines(data)]
    i, n = 0, len(lines)
    while i < n:
        desc = lines[i]
        i += 1
        if fasta:
            desc = b"@" + desc[1:]
            read = bytearray()
            while i < n and lines[i][0:1] != b">":
                read += lines[i]
                i += 1
            yield desc, bytes(read), None
        else:
            read = bytearray(lines[i])
            i += 1
            while lines[i][0:1] != b"+":
                read += lines[i]
                i += 1
            i += 1
            qual = bytearray(lines[i])
            i += 1
            while len(qual) < len(read) and i < n:
                qual += lines[i]
                i += 1
            yield desc, bytes(read), bytes(qual)


def starts_with(desc, key):
    """ByteArrayUtil.startsWith(readDescriptor, 1, key): the descriptor is NUL-terminated behind its last byte"""
    d = desc[1:]
    return len(d) >= len(key) and d[:len(key)] == key


def extract(data, key, fasta=False, with_probs=True):
    """-> (the bytes ExtractGoal writes, reads written); with_probs=False: ReadEntry.write of a reader that keeps no qualities
    (readProbs == null: '~' per base of the read), which the goal itself never asks for"""
    out = bytearray()
    n = 0
    for desc, read, qual in read_entries(data, fasta):
        if starts_with(desc, key):
            n += 1
            out += desc + b"\n" + read + b"\n+\n" + (qual if qual is not None and with_probs else b"~" * len(read)) + b"\n"
    return bytes(out), n
