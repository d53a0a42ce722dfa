"""A small Python model of kmer_build_vf6 (the probe-database builder): three phases over a sparse dict of table cells,
so any table size works, 2^35 cells included.  It is the yardstick of the GPU builder: tests/test_build_model.py pins it
to the recorded outputs of the reference (tests/golden/build_vf6), the GPU tests compare the builder with it.

Cell value: target << 11 | count (0 = empty, 1 = spoiled).  Only stdlib: math.log10 is the C library's log10.
"""
import gzip
import math
import os
import tarfile

K = 30
MASK = (1 << (2 * K)) - 1
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
BASES = "ACGT"
MAXREP = 2048
REPSHIFT = 11
BUFLEN = 0x4000


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_vf6")


def unpack_fixtures(dst):
    """golden/build_vf6/fixtures.tar.gz -> dst/in (the genome set), dst/out/<config> (what the reference wrote)"""
    with tarfile.open(os.path.join(GOLD, "fixtures.tar.gz")) as t:
        t.extractall(dst)


class Fatal(Exception):
    def __init__(self, code, message=""):
        super().__init__(message)
        self.code = code
        self.message = message


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & 0xFFFFFFFFFFFFFFFF
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & 0xFFFFFFFFFFFFFFFF
    k ^= k >> 33
    return k


def kmer_str(key):
    return "".join(BASES[(key >> (2 * (K - 1 - i))) & 3] for i in range(K))


# ---- sequence text ------------------------------------------------------------------------------------------------
def clean(line):
    """acgt/ACGT -> upper case, anything else -> N"""
    return "".join(c.upper() if c in "acgtACGT" else "N" for c in line)


def gz_text(data):
    """The .gz reader: '\\r' dropped at line end, a '>' line is one N, the unterminated last line is dropped, a line of
    16 KiB or more is fatal (exit 255)."""
    parts = data.split(b"\n")
    out = []
    for i, raw in enumerate(parts):
        if len(raw) >= BUFLEN:
            raise Fatal(255, "Buffer to small for input line lengths")
        if i == len(parts) - 1:
            break  # no '\n' behind it
        line = raw.decode("latin-1")
        if line.endswith("\r"):
            line = line[:-1]
        if line:
            out.append("N" if line[0] == ">" else clean(line))
    return "".join(out)


def contigs_text(data):
    """_contigs.fasta: all whitespace removed, lines of length <= 1 skipped."""
    out = []
    for raw in data.decode("latin-1").split("\n"):
        line = "".join(c for c in raw if c not in " \t\n\v\f\r")
        if len(line) > 1:
            out.append("N" if line[0] == ">" else clean(line))
    return "".join(out)


def read_gz(path):
    with open(path, "rb") as f:
        return gz_text(gzip.decompress(f.read()))


# ---- k-mers -------------------------------------------------------------------------------------------------------
def kmers(seq):
    """(gpos, keyF, keyR) of every 30-mer of ACGT bases; gpos = index of its last base"""
    cpos = f = r = 0
    for gpos, c in enumerate(seq):
        v = CODE.get(c)
        if v is None:
            cpos = f = r = 0
            continue
        f = ((f << 2) & MASK) | v
        r = (r >> 2) | ((3 - v) << (2 * (K - 1)))
        cpos += 1
        if cpos == K:
            yield gpos, f, r
            cpos -= 1


class Tree:
    def __init__(self, ntar):
        self.parent = [1] * ntar

    def add_edge(self, x, y):
        if 0 <= x < len(self.parent) and 0 <= y < len(self.parent):
            self.parent[y] = x

    def ca(self, x, y):
        anc = {1}
        z = x
        while z > 1:
            anc.add(z)
            z = self.parent[z]
        z = y
        while z not in anc:
            z = self.parent[z]
        return z


class Table:
    def __init__(self, log2_cells, tree):
        self.mask = (1 << log2_cells) - 1
        self.cells = {}
        self.size = 0
        self.tree = tree

    def index(self, key):
        return fmix64(key) & self.mask

    def add(self, key, targ):
        i = self.index(key)
        v = self.cells.get(i, 0)
        if v == 0:
            self.cells[i] = (targ << REPSHIFT) | 1
            self.size += 1
        elif (v >> REPSHIFT) > 1:
            t = self.tree.ca(v >> REPSHIFT, targ)
            c = v & (MAXREP - 1)
            self.cells[i] = 1 if c == MAXREP - 1 else (t << REPSHIFT) | (c + 1)

    def remove(self, key):
        i = self.index(key)
        if self.cells.get(i, 0) > 1:
            self.cells[i] = 1

    def take(self, key):
        i = self.index(key)
        v = self.cells.get(i, 0)
        self.cells[i] = 1
        return v >> REPSHIFT, v & (MAXREP - 1)


def add_seq(table, seq, targ):
    for _, f, r in kmers(seq):
        table.add(min(f, r), targ)


def remove_seq(table, seq):
    for _, f, r in kmers(seq):
        table.remove(min(f, r))


def minct(n):
    if n == 1:
        return 1
    if n < 4:
        return 2
    if n < 10:
        return n - 2
    return n // 5 + 1


_LOG10_4 = math.log10(4.0)


def entropy_flags(key):
    """(passes, bad) of the reference's check_entropy for the 30-mer `key`: fails on a run of 12+ equal bases or a frame
    entropy (mod 2, 3, 5; pseudo-count 1; log10; double) whose mean is below 0.80; `bad` k-mers are printed."""
    s = kmer_str(key)
    row = maxrow = 0
    prev = "N"
    for c in s:
        if c == prev:
            row += 1
            maxrow = max(maxrow, row)
        else:
            row, prev = 1, c
    if maxrow > 11:
        return False, False
    cnt = [[1.0] * 4 for _ in range(10)]
    for i, c in enumerate(s):
        b = CODE[c]
        cnt[i % 2][b] += 1.0
        cnt[i % 3 + 2][b] += 1.0
        cnt[i % 5 + 5][b] += 1.0
    ent = []
    for row4 in cnt:
        tot = row4[0] + row4[1] + row4[2] + row4[3]
        p = [x / tot for x in row4]
        e = -p[0] * math.log10(p[0])
        e = e - p[1] * math.log10(p[1])
        e = e - p[2] * math.log10(p[2])
        e = e - p[3] * math.log10(p[3])
        ent.append(e)
    e2 = (ent[0] + ent[1]) / 2.0 / _LOG10_4
    e3 = (ent[2] + ent[3] + ent[4]) / 3.0 / _LOG10_4
    e5 = (ent[5] + ent[6] + ent[7] + ent[8] + ent[9]) / 5.0 / _LOG10_4
    if e2 < 0.80 or e3 < 0.80 or e5 < 0.80:
        return False, False
    bad = (key & 0x3333333333333333) == 0 or (key & 0xCCCCCCCCCCCCCCCC) == 0
    return True, bad


def emit_seq(table, seq, org, ntargorgs, pcount, max_probes, out, stdout):
    minpos = -1
    n = 0
    for gpos, f, r in kmers(seq):
        key = min(f, r)
        t, c = table.take(key)
        if t > 1 and c >= minct(ntargorgs[t]) and gpos > minpos and pcount[t] < max_probes:
            ok, bad = entropy_flags(key)
            if ok:
                if bad:
                    stdout.append(kmer_str(key) + "\n")
                out.append("%s,%d,%d,%d,%s,%d\n" % (kmer_str(key), t, org, gpos, "F" if f < r else "R", c))
                minpos = gpos + K
                pcount[t] += 1
                n += 1
    return n


# ---- the program --------------------------------------------------------------------------------------------------
def _read_lines(path):
    """getline() over a file (a final line without '\\n' included); None if it cannot be opened"""
    try:
        data = open(path, "rb").read().decode("latin-1")
    except OSError:
        return None
    lines = data.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def run(cwd, name=None, fadir="", genbank_dir="/mnt/dmb/Mark_backup/genbank/", log2_cells=35, max_probes=100000):
    """Runs the builder in directory `cwd` like `kmer_build_vf6 -name NAME -fadir FADIR` (name=None: no -name, "bob").
    Returns (exit_status, stdout_text, stderr_text); writes NAME/NAME_probes.txt and NAME/NAME_count.txt like it."""
    wdir = os.path.join(cwd, name) + "/" if name is not None else cwd + "/"
    name = name if name is not None else "bob"

    def p(rel):
        return rel if os.path.isabs(rel) else os.path.join(cwd, rel)

    stdout = []
    outs = []
    for line in _read_lines(wdir + name + "_filter.txt") or []:
        w = line.split()
        outs.append(w[0] if w else (outs[-1] if outs else ""))
    stdout.append("%d outs loaded\n" % len(outs))
    targno, acc = [], []
    for line in _read_lines(wdir + name + "_data.txt") or []:
        w = line.split()
        targno.append(int(w[0]))
        acc.append(w[1])
    num_targ = max([0] + targno) + 1
    stdout.append("%d sequences loaded\n" % len(acc))
    ntargorgs = [0] * num_targ
    pcount = [0] * num_targ
    for t in targno:
        if t > 1:
            ntargorgs[t] += 1
    tree = Tree(num_targ)
    for line in _read_lines(wdir + name + "_tree.txt") or []:
        w = line.split()
        if len(w) >= 2:
            tree.add_edge(int(w[0]), int(w[1]))
    stdout.append("tree loaded\n")
    probes = []
    probes_path = wdir + name + "_probes.txt"
    open(probes_path, "w").close()
    table = Table(log2_cells, tree)
    fa, gb = p(fadir), p(genbank_dir)

    def load(cands):
        for path, kind in cands:
            if os.path.exists(path):
                data = open(path, "rb").read()
                if kind == "gz":
                    return gz_text(gzip.decompress(data))
                return contigs_text(data)
        return None

    try:
        n = len(acc)
        for i in range(n):
            if targno[i] <= 1:
                continue
            seq = load([(fa + acc[i] + ".fasta.gz", "gz"), (gb + acc[i] + ".fasta.gz", "gz"), (fa + acc[i] + "_contigs.fasta", "fa")])
            if seq is None:
                stdout.append("no file for %s\n" % acc[i])
                raise Fatal(1)
            stdout.append("1 %d %d %s\n" % (i, n, acc[i]))
            add_seq(table, seq, targno[i])
        stdout.append("\n")
        for i, a in enumerate(outs):
            seq = load([(gb + a + ".fasta.gz", "gz"), (fa + a + ".fasta.gz", "gz")])
            if seq is None:
                stdout.append("no file for %s\n" % a)
                raise Fatal(1)
            stdout.append("2 %d %d %s\n" % (i, len(outs), a))
            remove_seq(table, seq)
        stdout.append("\n")
        tct = 0
        for i in range(n):
            if targno[i] <= 1:
                continue
            seq = load([(fa + acc[i] + ".fasta.gz", "gz"), (gb + acc[i] + ".fna.gz", "gz"), (fa + acc[i] + "_contigs.fasta", "fa")])
            if seq is None:
                stdout.append("no file for %s\n" % acc[i])
                raise Fatal(1)
            stdout.append("3 %d %d %s\n" % (i, n, acc[i]))
            tct += emit_seq(table, seq, i, ntargorgs, pcount, max_probes, probes, stdout)
    except Fatal as e:
        with open(probes_path, "w") as f:
            f.write("".join(probes))
        return e.code, "".join(stdout), (e.message + "\n") if e.message else ""
    with open(probes_path, "w") as f:
        f.write("".join(probes))
    stdout.append("\n")
    with open(wdir + name + "_count.txt", "w") as f:
        f.write("".join("%d,%d\n" % (i, pcount[i]) for i in range(num_targ)))
    stdout.append("probe count %d\n" % tct)
    stdout.append("size %d\n" % table.size)
    return 0, "".join(stdout), ""
