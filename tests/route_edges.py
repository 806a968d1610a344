"""Short-read junction batches whose consensus length m and window length n = |svRefStr| are chosen exactly: the shapes on
which build_bins (delly_amd/csrc/dellyhip.hip) picks a kernel for a junction.

  split_sparse_kernel       m <= SPS_MMAX = 254, n <= SPS_NMAX = 1280, n + m + 1 <= SPS_ND = 1536, ACGTN only
  split_sparse_wide_kernel  the rest up to m <= MMAX = 319, n <= NMAX = 2048 (ACGTN only)
  split_quad_kernel<KQ, KP> m + 1 <= 160, n <= QNMAX = 1280; KQ = ceil((m + 1) / 32), KP = (KQ + 1) / 2 merged in
  split_pair_kernel<K>      the rest up to m = 319, K = ceil((m + 1) / 64)
  split_align_kernel<K>     a packed seat whose consensus has more than 15 distinct bytes
  strip kernel              m >= 320 or n >= 2049

Windows (src/split.h:70-163, mirrored by host_window_len):
  DEL, svEnd - svStart <= indelsize: one window svStart - m .. svEnd + m, n = span + 2 m (the contiguous branch)
  DEL beyond indelsize, DUP, INV beyond minConsWindow: two windows of 2 m each when span >= 2 m, n = 4 m
  DEL on a chromosome shorter than 2 m + span: the window is clamped at both ends, n = the chromosome's length
With the `delly sr` default indelsize of 1000 the contiguous branch reaches n = 2 m + 1000 only; a cell beyond that is
generated for indelsize = WIDE_INDELSIZE (params_for).  Every junction is a real split at a known breakpoint (the consensus
is the ALT haplotype, its two flanks ending and starting exactly at the breakpoints), optionally made noisy:
  "sub"   20 % substitutions: far beyond the sparse kernels' 32 deficit levels, the dense kernels finish it
  "lower" a few lower-case letters: not ACGTN, neither sparse kernel takes it
Junction k of a batch depends on (seed, k) only."""
import numpy as np

from delly_amd import abi, synth

GRID_M = [31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 253, 254, 255, 256, 318, 319]
GRID_N = [1279, 1280, 1281, 2047, 2048, 2049]
CORNERS = [(254, 1280), (254, 1281), (255, 1280), (319, 2048)]
WIDE_INDELSIZE = 2048
TWO_WINDOW_SPAN = 2500       # > WIDE_INDELSIZE: the two-window branch under either indelsize
TWO_WINDOW_KINDS = ("del2", "dup", "inv0", "inv1")
NOISE = ("clean", "sub", "lower")

# bytes beyond ACGT for the wide-alphabet consensus: upper / lower IUPAC, punctuation, bytes >= 0x80 (never NUL)
EXTRA = (b"RYKMSWBDHVN" + b"acgtnrykmswbdhv" + b"!#$%&*+-./:;<=>?@^_~" + bytes(range(0x80, 0xff, 5)))
assert len(set(EXTRA)) == len(EXTRA) and 0 not in EXTRA and not set(EXTRA) & set(b"ACGT")


def span_of(kind, m, n):
    """the breakpoint distance svEnd - svStart that gives junction kind at consensus length m a window of exactly n"""
    if kind == "del":
        assert n >= 2 * m, (m, n)
        return n - 2 * m
    assert n == 4 * m, (kind, m, n)
    return TWO_WINDOW_SPAN


def params_for(kind, m, n):
    """`delly sr` defaults, or indelsize raised to WIDE_INDELSIZE where the contiguous window needs a longer deletion"""
    p = abi.params_sr()
    if kind == "del" and span_of(kind, m, n) > p.indelsize:
        p.indelsize = WIDE_INDELSIZE
    return p


def _noise(rng, cons, noise):
    c = cons.copy()
    if noise == "sub":
        hit = rng.random(c.size) < 0.2
        c[hit] = synth.ACGT[rng.integers(0, 4, int(hit.sum()))]
    elif noise == "lower":
        at = rng.choice(c.size, size=min(3, c.size), replace=False)
        c[at] |= 0x20
    return c


def _alphabet(rng, G, pos, distinct):
    """writes bytes into G at the genome positions `pos` of a consensus (in consensus order) so that the consensus holds exactly
    `distinct` different bytes: A, C, G, T once each at four positions, EXTRA[:distinct - 4] at the others"""
    m = len(pos)
    assert 4 <= distinct <= min(m, 4 + len(EXTRA)), (m, distinct)
    slots = rng.permutation(m)
    for i, ch in enumerate(b"ACGT"):
        G[pos[slots[i]]] = ch
    extra = np.frombuffer(EXTRA[:distinct - 4], dtype=np.uint8)
    rest = slots[4:]
    G[pos[rest[:extra.size]]] = extra                         # every extra byte at least once
    tail = rest[extra.size:]
    pool = np.concatenate([synth.ACGT, extra])
    G[pos[tail]] = pool[rng.integers(0, pool.size, tail.size)]


def make(cells, *, seed=1, distinct=None):
    """cells: list of (m, n, kind, noise, count).  kind "del" (contiguous DEL, any n >= 2 m), "del2" / "dup" / "inv0" / "inv1"
    (n = 4 m), "tiny" (a DEL on a chromosome of n < 2 m letters: the window is the chromosome).  distinct: None, or per cell a
    number of distinct consensus bytes (ACGT + EXTRA bytes, written into the genome too; a third of the extra bytes face the next
    byte of the alphabet there instead, so that a kernel which merged two letter codes would score them as matches).
    -> synth.Batch; truth[k] = dict(m, n, kind, noise, distinct)"""
    rows = []
    for ci, (m, n, kind, noise, count) in enumerate(cells):
        for _ in range(count):
            rows.append((m, n, kind, noise, distinct[ci] if distinct is not None else None))
    k_big = [k for k, r in enumerate(rows) if r[2] != "tiny"]
    W = max([2 * r[0] + span_of(r[2], r[0], r[1]) for r in rows if r[2] != "tiny"] + [0]) + 600
    chrom = np.empty(len(k_big) * W, dtype=np.uint8)
    chroms = [chrom]
    junc = np.zeros(len(rows), dtype=abi.junction_dtype())
    seqs, truth = [], []
    slot = 0
    for k, (m, n, kind, noise, dist) in enumerate(rows):
        rng = synth._rng(seed, k)
        fl = int(rng.integers(m // 3, m - m // 3 + 1))       # a breakpoint in the middle third of the consensus
        fr = m - fl
        if kind == "tiny":
            assert n < 2 * m
            c = synth.ACGT[rng.integers(0, 4, n)]
            chroms.append(c)
            cons = synth.ACGT[rng.integers(0, 4, m)]
            junc[k]["chr"] = junc[k]["chr2"] = len(chroms) - 1
            junc[k]["svt"] = 2
            junc[k]["sv_start"] = n // 2
            junc[k]["sv_end"] = n - n // 2 if n > 1 else 1
            if junc[k]["sv_end"] < junc[k]["sv_start"]:
                junc[k]["sv_end"] = junc[k]["sv_start"]
        else:
            G = synth.ACGT[rng.integers(0, 4, W)]
            span = span_of(kind, m, n)
            s = m + 300
            e = s + span
            if kind in ("del", "del2"):
                pos = np.concatenate([np.arange(s - fl, s), np.arange(e, e + fr)])
                svt = 2
            elif kind == "dup":
                pos = np.concatenate([np.arange(e - fl, e), np.arange(s, s + fr)])
                svt = 3
            elif kind == "inv0":          # 3to3: left flank, then the reverse complement of the sequence before svEnd
                pos = np.concatenate([np.arange(s - fl, s), np.arange(e - 1, e - fr - 1, -1)])
                svt = 0
            else:                         # inv1, 5to5: the reverse complement of the sequence from svStart, then the right flank
                pos = np.concatenate([np.arange(s + fl - 1, s - 1, -1), np.arange(e, e + fr)])
                svt = 1
            if dist is not None:
                _alphabet(rng, G, pos, dist)
            cons = G[pos].copy()
            if dist is not None:
                # a third of the extra bytes face the next byte of the alphabet in the genome (byte order is the order of the
                # kernels' letter codes): two adjacent codes merged would match
                ex = np.frombuffer(EXTRA[:dist - 4], dtype=np.uint8)
                alpha = np.sort(np.concatenate([synth.ACGT, ex]))
                nxt = np.arange(256, dtype=np.uint8)
                nxt[alpha] = np.roll(alpha, -1)
                at = np.nonzero(np.isin(cons, ex) & (rng.random(m) < 1 / 3))[0]
                G[pos[at]] = nxt[cons[at]]
            if kind == "inv0":
                cons[fl:] = synth._COMP[cons[fl:]]
            elif kind == "inv1":
                cons[:fl] = synth._COMP[cons[:fl]]
            chrom[slot * W:(slot + 1) * W] = G
            junc[k]["svt"] = svt
            junc[k]["sv_start"] = slot * W + s
            junc[k]["sv_end"] = slot * W + e
            slot += 1
        cons = _noise(rng, cons, noise)
        assert cons.size == m
        junc[k]["svid"] = k
        junc[k]["seq_first"] = k
        junc[k]["n_seq"] = 1
        seqs.append(cons)
        truth.append(dict(m=m, n=n, kind=kind, noise=noise, distinct=dist))
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([x.size for x in seqs])
    return synth.Batch(chroms, junc, np.concatenate(seqs), off, 0, truth)


def grid_cells(per_noise=(3, 1, 1)):
    """the shape grid: every m of GRID_M at every n of GRID_N (contiguous DEL), and at n = 4 m through each two-window kind,
    grouped by the indelsize they need -> {"default": cells, "wide": cells}"""
    out = {"default": [], "wide": []}
    for m in GRID_M:
        for n in GRID_N:
            group = "wide" if params_for("del", m, n).indelsize != abi.params_sr().indelsize else "default"
            for noise, c in zip(NOISE, per_noise):
                if c:
                    out[group].append((m, n, "del", noise, c))
        for kind in TWO_WINDOW_KINDS:
            for noise, c in zip(NOISE, per_noise):
                if c:
                    out["default"].append((m, 4 * m, kind, noise, c))
    return out


def grid_batches(seed=11):
    """-> {label: (batch, params)} of grid_cells()"""
    out = {}
    for i, (label, cells) in enumerate(sorted(grid_cells().items())):
        p = abi.params_sr()
        if label == "wide":
            p.indelsize = WIDE_INDELSIZE
        out[label] = (make(cells, seed=seed + i), p)
    return out


DEFER_M = [31, 63, 95, 127, 159, 191, 254, 318]
DEFER_D = [15, 16, 17, 60]


def deferral_batch(seed=21):
    """per m of DEFER_M (quad bins 1 .. 5 and pair bins 3 .. 5; pair bins 1 .. 3 with the quad kernel off) and per number of
    distinct consensus bytes of DEFER_D: one wide-alphabet junction and three ordinary ACGT partners of the same shape, in
    this order, its seat in the group of four turning with the cell -- one window per m, so that a bin's stable sort by window
    keeps them side by side: the wide-alphabet junction shares its pair / quad wavefront with ordinary junctions"""
    cells, dist = [], []
    for m in DEFER_M:
        n = 2 * m + 400
        for i, d in enumerate(D for D in DEFER_D if D <= m):
            group = [(m, n, "del", "clean", 1, d)] + [(m, n, "del", "clean", 1, None)] * 3
            group = group[-(i % 4):] + group[:-(i % 4)] if i % 4 else group
            for c in group:
                cells.append(c[:5])
                dist.append(c[5])
    return make(cells, seed=seed, distinct=dist)


SEAT_QUAD_M = [31, 63, 95, 127, 159]
SEAT_PAIR_M = [191, 254, 318]


def seat_batch(quad_count, pair_count, seed=31):
    """per quad bin (SEAT_QUAD_M) quad_count junctions and per pair-only bin (SEAT_PAIR_M) pair_count junctions, windows
    sorted down the bin's seats: the largest a quad / pair seat takes, one equal to it, then 2 m + 7, then 3, 2, 1, ...
    letters (tiny chromosomes), so that partners sit at nB = nA, nB << nA and nB <= 3 and the last seats are empty"""
    cells = []
    for ms, count, top in ((SEAT_QUAD_M, quad_count, 1280), (SEAT_PAIR_M, pair_count, 2048)):
        for m in ms:
            ns = [top, top, 2 * m + 7] + [3, 2, 1, 3, 2, 1]
            for i in range(count):
                n = ns[i] if i < len(ns) else 2 * m + 7 + i
                cells.append((m, n, "del" if n >= 2 * m else "tiny", "clean", 1))
    return make(cells, seed=seed + 97 * quad_count + pair_count)


def wide_kernel_batch(n, seed=41):
    """n clean junctions beyond the byte tile and within the wide kernel: m 255 .. 319 and n 1281 .. 2048 in turn"""
    rng = np.random.default_rng(seed)
    cells = []
    for k in range(n):
        m = int(rng.integers(255, 320)) if k % 2 else int(rng.integers(200, 320))
        w = int(rng.integers(max(1281, 2 * m), 2049)) if k % 2 == 0 else int(rng.integers(2 * m, 2049))
        cells.append((m, w, "del", "clean", 1))
    return make(cells, seed=seed)


COUNTER_CELLS = [(254, 1280, "del", "clean", 6), (253, 1280, "del", "clean", 3), (255, 1280, "del", "clean", 4),
                 (254, 1281, "del", "clean", 4), (319, 2048, "del", "clean", 3), (254, 1280, "del", "lower", 3),
                 (255, 1280, "del", "lower", 4), (254, 1281, "del", "lower", 5), (319, 2049, "del", "lower", 2)]


def counter_batch(seed=5):
    """clean and lower-case junctions on both sides of the byte tile's and the wide kernel's limits (indelsize WIDE_INDELSIZE)"""
    return make(COUNTER_CELLS, seed=seed)


def windows(batch):
    """(consensus, |svRefStr| bytes) per junction for the single-item long_needle: the window of the contiguous branch"""
    out = []
    for k in range(batch.n):
        j = batch.junctions[k]
        m = int(batch.seq_off[k + 1] - batch.seq_off[k])
        c = batch.chroms[int(j["chr"])]
        a, b = max(0, int(j["sv_start"]) - m), min(c.size, int(j["sv_end"]) + m)
        out.append((bytes(batch.seq_blob[int(batch.seq_off[k]):int(batch.seq_off[k + 1])]), bytes(c[a:b])))
    return out
