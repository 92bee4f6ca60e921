"""The taxtree and taxnodes goals in plain Python, written from the reference's Java: TaxTree(File, boolean)
(C/tax/TaxTree.java:92-122, readNodesFromStream :226-254, readNamesFromStream :196-216, initPositions :491-502) over
BufferedLineReader.nextLine (B/io/BufferedLineReader.java:160-182) and DigitTrie (C/util/DigitTrie.java:106-189); TaxIdCollector
(C/tax/TaxIdCollector.java:67-126,172-185) under TaxNodesGoal (C/goals/TaxNodesGoal.java:74-94); TaxIdNode.markRequired
(TaxTree.java:536-544), SmallTaxTree(TaxTree) (C/tax/SmallTaxTree.java:60-64, 427-454) and Database.initStoreIndices
(C/store/Database.java:107-128) on a store without values.

A node is its index in the ascending array of distinct tax ids.  The reference keys nodes by the STRING of the id: "01" and ""
(a bar in column 1) would be nodes of their own there.  Tax ids are int32 here, so such a line raises Unsupported; so does an id
of more than nine digits.  Where the reference throws, Throws carries the 1-based line."""
import numpy as np

MAX_LINE_SIZE = 4096

RANK_NAMES = ("cellular root", "acellular root", "superkingdom", "domain", "realm", "kingdom", "phylum", "subphylum", "superclass", "class",
              "subclass", "superorder", "order", "suborder", "superfamily", "family", "subfamily", "tribe", "genus", "subgenus",
              "species group", "species", "varietas", "subspecies", "serogroup", "biotype", "strain", "serotype", "genotype", "forma",
              "forma specialis", "isolate", "clade", "no rank", "subkingdom", "section", "REFINED", "DATA", "FILE", "ID")
# Rank(String): level = ordinal * 20; clade and no rank: -1; subkingdom: kingdom + 10; section: genus + 10
RANK_LEVELS = [i * 20 for i in range(len(RANK_NAMES))]
RANK_LEVELS[RANK_NAMES.index("clade")] = RANK_LEVELS[RANK_NAMES.index("no rank")] = -1
RANK_LEVELS[RANK_NAMES.index("subkingdom")] = RANK_LEVELS[RANK_NAMES.index("kingdom")] + 10
RANK_LEVELS[RANK_NAMES.index("section")] = RANK_LEVELS[RANK_NAMES.index("genus")] + 10


class Throws(Exception):
    """the reference throws here"""

    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


class Unsupported(Exception):
    """the reference goes on, with a node that an int32 tax id cannot name"""

    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def next_lines(data):
    """BufferedLineReader.nextLine over the whole stream -> [(bytes of target[0:min(size, 4096)], size)] up to the first size 0.
    NUL bytes are dropped, '\\r' stays, the newline is part of the line, and a line that fills the buffer answers 4097: its rest is
    read as the next line."""
    out, pos, n = [], 0, len(data)
    while True:
        buf = bytearray()
        c = -1
        while len(buf) < MAX_LINE_SIZE and pos < n and c != 10:
            c = data[pos]
            pos += 1
            if c != 0:
                buf.append(c)
        if c == 10:
            size = len(buf)
        elif len(buf) == MAX_LINE_SIZE and pos < n:
            size = MAX_LINE_SIZE + 1
        elif len(buf) == MAX_LINE_SIZE:
            # the buffer is full as the stream ends: the loop leaves with pos == bufferFill, `size == target.length` answers 4097
            size = MAX_LINE_SIZE + 1
        else:
            size = len(buf)
        if size <= 0:
            return out
        out.append((bytes(buf), size))


def _index_of(target, start, end, byte, line):
    """ByteArrayUtil.indexOf(array, start, end, char): reads array[4096] if end is 4097 and nothing is found in front of it"""
    for i in range(start, end):
        if i >= MAX_LINE_SIZE:
            raise Throws(line, "ArrayIndexOutOfBoundsException: no bar in a line that fills the buffer")
        if target[i] == byte:
            return i
    return -1


def _taxid(target, start, end, create, line):
    """DigitTrie.getNode over target[start, end): None: no node can have this key (a byte that is no digit); raises where the
    reference throws (create) or where the key is no int32 tax id of this library"""
    if end < start:
        if create:
            raise Throws(line, "StringIndexOutOfBoundsException: a key of negative length")
        return None  # (the trie's own root, which holds no value: an empty key is Unsupported at its create)
    key = target[start:end]
    if not all(48 <= b <= 57 for b in key):
        if create:
            raise Throws(line, "IllegalStateException: Cant get node via sequence")
        return None
    if len(key) == 0 or key[0] == 48 or len(key) > 9:
        if create:
            raise Unsupported(line, "an empty id, a leading zero or more than nine digits")
        return None  # (no line can have created it)
    return int(key)


def rank_of(field):
    """Rank.getRankFromBytes: the ordinal of the rank whose name equals the bytes, else -1"""
    try:
        return RANK_NAMES.index(field.decode("latin-1"))
    except ValueError:
        return -1


def nodes_slots(data, line0=0):
    """readNodesFromStream, its lines alone -> [(id, parent, rank ordinal)] of the lines that are not skipped, in order"""
    out = []
    for no, (target, size) in enumerate(next_lines(data), start=line0 + 1):
        a = _index_of(target, 0, size, 124, no)
        b = _index_of(target, a + 1, size, 124, no)
        c = _index_of(target, b + 1, size, 124, no)
        if a != -1 and b != -1:
            node_a = _taxid(target, 0, a - 1, True, no)
            node_b = _taxid(target, a + 2, b - 1, True, no)
            rank = rank_of(target[b + 2:c - 1]) if c - 1 >= b + 2 else -1
            out.append((node_a, node_b, rank))
    return out


class Tree:
    """the tree of readNodesFromStream and initPositions as arrays over the ascending distinct tax ids"""

    def __init__(self, slots):
        ids = sorted({s[0] for s in slots} | {s[1] for s in slots})
        self.taxids = np.array(ids, dtype=np.int32)
        index = {t: i for i, t in enumerate(ids)}
        n = len(ids)
        self.n = n
        self.parent = np.full(n, -1, dtype=np.int32)
        self.rank = np.full(n, -1, dtype=np.int32)
        self.children = [[] for _ in range(n)]
        self.duplicates = 0
        seen = set()
        root = None
        for tid, par, rank in slots:
            a, b = index[tid], index[par]
            self.duplicates += tid in seen
            seen.add(tid)
            if a != b:
                self.children[b].append(a)  # addSubNode: in line order; twice if two lines say so
                self.parent[a] = b
            self.rank[a] = rank
            if a == b and tid == 1:
                root = a
        if root is None:
            raise Throws(0, "NullPointerException: no root")
        self.root = root
        self.depth = np.full(n, -1, dtype=np.int32)
        self.position = np.full(n, -1, dtype=np.int32)
        self.subtree = np.zeros(n, dtype=np.int32)
        self.names = [None] * n
        # initPositions(0, 0), without the recursion
        counter = 0
        self.position[root], self.depth[root] = 0, 0
        stack, on_stack = [(root, 0)], {root}
        while stack:
            v, i = stack[-1]
            if i < len(self.children[v]):
                stack[-1] = (v, i + 1)
                c = self.children[v][i]
                if c in on_stack:
                    raise Throws(0, "StackOverflowError: a cycle that the root reaches")
                counter += 1
                self.position[c], self.depth[c] = counter, len(stack)
                stack.append((c, 0))
                on_stack.add(c)
            else:
                self.subtree[v] = counter - self.position[v] + 1
                stack.pop()
                on_stack.discard(v)

    def node_of(self, taxid):
        i = int(np.searchsorted(self.taxids, taxid))
        return i if i < self.n and self.taxids[i] == taxid else -1

    def read_names(self, data):
        """readNamesFromStream"""
        for no, (target, size) in enumerate(next_lines(data), start=1):
            scientific = _contains_scientific(target, size, no)
            a = _index_of(target, 0, size, 124, no)
            b = _index_of(target, a + 1, size, 124, no)
            if a != -1 and b != -1:
                tid = _taxid(target, 0, a - 1, False, no)
                node = self.node_of(tid) if tid is not None else -1
                if node >= 0:
                    if b - a - 3 < 0:
                        raise Throws(no, "StringIndexOutOfBoundsException: a name of negative length")
                    if self.names[node] is None or scientific:
                        self.names[node] = target[a + 2:b - 1]

    # ---- TaxIdCollector
    def _complete(self, starts, cut):
        """withDescendants(starts, cut): cut is a rank ordinal or None"""
        res = set()
        for s in starts:
            stack, on_stack = [(s, 0)], {s}
            res.add(s)
            while stack:
                v, i = stack[-1]
                if i < len(self.children[v]):
                    stack[-1] = (v, i + 1)
                    c = self.children[v][i]
                    if cut is None or (self.rank[c] != -1 and not is_below(int(self.rank[c]), cut)):
                        if c in on_stack:
                            raise Throws(0, "StackOverflowError: a requested node lies on a cycle")
                        res.add(c)
                        stack.append((c, 0))
                        on_stack.add(c)
                else:
                    stack.pop()
                    on_stack.discard(v)
        return res

    def select(self, requested, excluded, cut=None):
        """TaxNodesGoal.doMakeThis over node indices -> uint8[n]"""
        res = self._complete(set(requested), cut) - self._complete(set(excluded), None)
        out = np.zeros(self.n, dtype=np.uint8)
        out[sorted(res)] = 1
        return out

    def small_tree(self, flagged):
        """markRequired on every flagged node, SmallTaxTree(TaxTree), initStoreIndices on a store without values ->
        (node_of_vi, parent_vi, depth, position): the root is always there; position is the FULL tree's (SmallTaxTree.java:430)"""
        required = np.zeros(self.n, dtype=bool)
        for v in np.flatnonzero(np.asarray(flagged) > 0):
            v = int(v)
            while v != -1 and not required[v]:
                required[v] = True
                v = int(self.parent[v])
        node_of_vi, parent_vi = [self.root], [-1]
        vi_of = {self.root: 0}
        stack = [(self.root, 0)]
        while stack:
            v, i = stack[-1]
            if i < len(self.children[v]):
                stack[-1] = (v, i + 1)
                c = self.children[v][i]
                if required[c] and c not in vi_of:  # (getAddValueIndex: one index per tax id)
                    vi_of[c] = len(node_of_vi)
                    node_of_vi.append(c)
                    parent_vi.append(vi_of[v])
                    stack.append((c, 0))
            else:
                stack.pop()
        node_of_vi = np.array(node_of_vi, dtype=np.int32)
        return node_of_vi, np.array(parent_vi, dtype=np.int32), self.depth[node_of_vi], self.position[node_of_vi]


def _contains_scientific(target, size, line):
    """ByteArrayUtil.indexOf(target, 0, size, "scientific name") != -1"""
    pat = b"scientific name"
    for i in range(0, size - len(pat) + 1):
        for j in range(len(pat)):
            if i + j >= MAX_LINE_SIZE:
                raise Throws(line, "ArrayIndexOutOfBoundsException")
            if target[i + j] != pat[j]:
                break
        else:
            return True
    return False


def is_below(rank, other):
    """Rank.isBelow over ordinals"""
    a, b = RANK_LEVELS[rank], RANK_LEVELS[other]
    return a != -1 and b != -1 and a > b


def read_taxids(text):
    """TaxIdCollector.readFromFile, the strings alone -> (requested, excluded) as lists of str, in file order.  BufferedReader.readLine
    ends a line at \\n, \\r or \\r\\n; String.trim drops everything up to U+0020 at both ends."""
    requested, excluded = [], []
    for line in text.decode("utf-8", "replace").replace("\r\n", "\n").replace("\r", "\n").split("\n"):
        line = _trim(line)
        if line.startswith("#"):
            continue
        k = line.find("#")
        if k != -1:
            line = line[:k]
        tab = line.rfind("\t")
        taxid = _trim(line[tab:] if tab != -1 else line)
        if taxid:
            (excluded if taxid.startswith("-") else requested).append(taxid[1:] if taxid.startswith("-") else taxid)
    return requested, excluded


def _trim(s):
    a, b = 0, len(s)
    while a < b and s[a] <= " ":
        a += 1
    while b > a and s[b - 1] <= " ":
        b -= 1
    return s[a:b]


def taxid_nodes(tree, strings):
    """getNodeByTaxId per string: a string that is no id of a node is dropped"""
    out = []
    for s in strings:
        if s and s.isascii() and s.isdigit() and s[0] != "0" and len(s) <= 9 and tree.node_of(int(s)) >= 0:
            out.append(tree.node_of(int(s)))
    return out


def in_nodes_grammar(line):
    """the device's grammar of a nodes line, its newline included (gs_taxtree.hip)"""
    if line == b"\n":
        return True
    if len(line) > MAX_LINE_SIZE or 0 in line or line.count(b"|") < 3:
        return False
    a = line.index(b"|")
    b = line.index(b"|", a + 1)
    tid, par = line[:max(a - 1, 0)], line[a + 2:max(b - 1, a + 2)]
    ok = lambda f: 1 <= len(f) <= 9 and f.isdigit() and f[0] != 48
    return a >= 1 and b - 1 >= a + 2 and ok(tid) and ok(par)
