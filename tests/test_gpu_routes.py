"""-m gpu: every short-read kernel route of build_bins (delly_amd/csrc/dellyhip.hip) against the reference itself (oracle/_ref),
on junctions whose consensus length m and window length n = |svRefStr| sit exactly on the limits that choose the route
(tests/route_edges.py; tests/test_oracle_golden.py pins m and n through the C restatement):

  split_sparse_kernel        m <= 254, n <= 1280, n + m + 1 <= 1536, ACGTN only, deficit <= 32 levels
  split_sparse_wide_kernel   beyond that, m <= 319, n <= 2048 (DELLYHIP_SR_WIDE)
  split_quad_kernel<KQ, KP>  m + 1 <= 160, n <= QNMAX = 1280 (DELLYHIP_QUAD; DELLYHIP_QUAD_MIX seats small bins as pair items)
  split_pair_kernel<K>       the rest up to m = 319
  split_align_kernel<K>      a packed seat whose consensus holds more than 15 distinct bytes (DH_DEFERRED)
  strip kernel               m >= 320 or n >= 2049

The knob matrix (KNOBS) moves every grid junction from one route to the next: with DELLYHIP_SR_SPARSE=0 the clean junctions the
sparse kernels take by default go to the quad / pair kernels, with DELLYHIP_QUAD=0 as well the quad bins go to the pair kernel,
with DELLYHIP_SR_WIDE=0 what the wide kernel finishes goes to the dense kernels.  All configurations must give the reference's
records and bytes, and so each other's.  Where a counter shows the route (ResidentBatch.sparse_left: what the two sparse kernels
left behind) test_route_counters asserts it."""
import os

import numpy as np
import pytest

import route_edges as R
from delly_amd import abi, refine, synth
from util import CORE, INTERNAL, compare

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 1, 64)

KNOBS = {
    "default": {},
    "dense": {"DELLYHIP_SR_SPARSE": "0"},                             # quad + pair
    "pair": {"DELLYHIP_SR_SPARSE": "0", "DELLYHIP_QUAD": "0"},        # pair only
    "nowide": {"DELLYHIP_SR_WIDE": "0"},                              # byte tile, then the dense kernels
    "quadmix": {"DELLYHIP_QUAD_MIX": "1"},
    "dense-quadmix": {"DELLYHIP_SR_SPARSE": "0", "DELLYHIP_QUAD_MIX": "1"},   # quad bins as pair items of split_quad_kernel
}


def wide_params():
    p = abi.params_sr()
    p.indelsize = R.WIDE_INDELSIZE
    return p


class _Env:
    """the knobs are read at dellyhip_create: set them around Context()"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def context(p, env):
    with _Env(env):
        return refine.Context(params=p)


def gpu_refine(batch, p, env, want_alignment):
    ctx = context(p, env)
    try:
        ctx.set_chromosomes(batch.chroms)
        return ctx.refine(batch, want_alignment=want_alignment)
    finally:
        ctx.close()


def _fields(want, internal=False):
    return [f for f in CORE + (INTERNAL if internal else []) if want or f != "aln_len"]


def _blobs(want):
    return ("cons", "allele", "aln") if want else ("cons", "allele")


_REF = {}


def expected(reference, port, label, batch, p):
    """(reference records + blob, port records + blob) of a batch, once per session: the reference for CORE and the bytes, the C
    restatement (which tests/test_oracle_golden.py holds to the reference on these batches) for the INTERNAL fields"""
    if label not in _REF:
        _REF[label] = (reference.refine_batch(batch, params=p, want_alignment=True, n_threads=THREADS),
                       port.refine_batch(batch, params=p, want_alignment=True, n_threads=THREADS))
    return _REF[label]


def check_all(reference, port, label, batch, p, got, want):
    (rr, rb), (pr, pb) = expected(reference, port, label, batch, p)
    gr, gb = got
    compare(gr, gb, rr, rb, fields=_fields(want), blobs=_blobs(want), label=label + " vs reference")
    compare(gr, gb, pr, pb, fields=_fields(want, True), blobs=(), label=label + " vs restatement")


GRID = R.grid_batches()


# ---- the shape grid under the knob matrix -----------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(GRID))
def test_shape_grid_under_every_route_knob(reference, port, group):
    """m at every quad-bin edge (m + 1 = 32/33 .. 160/161), pair-bin edge (64/65 .. 256/257), the byte tile's m = 254/255 and
    MMAX = 318/319; n at SPS_NMAX = QNMAX = 1279/1280/1281 and NMAX = 2047/2048/2049 (contiguous DEL; group "wide" holds the cells
    whose deletion needs indelsize 2048), and n = 4 m through the two-window DEL / DUP / INV 3to3 / INV 5to5 windows; clean,
    20 % substituted and lower-case copies.  Every knob configuration, with and without alignment rows, is the reference's,
    and all configurations agree on every CORE + INTERNAL field and byte."""
    b, p = GRID[group]
    (rr, _), _ = expected(reference, port, "grid " + group, b, p)
    assert int(rr["ok"].sum()) >= b.n // 3
    for want in (False, True):
        first = None
        for name, env in KNOBS.items():
            got = gpu_refine(b, p, env, want)
            check_all(reference, port, "grid %s %s aln=%d" % (group, name, want), b, p, got, want)
            if first is None:
                first = got
            else:
                compare(got[0], got[1], first[0], first[1], fields=_fields(want, True), blobs=_blobs(want),
                        label="grid %s %s vs default aln=%d" % (group, name, want))


def test_route_counters(reference):
    """ResidentBatch.sparse_left() counts what the two sparse kernels were offered and left behind.  Lower-case letters make
    every sparse kernel leave a junction, so the count says which junctions were offered to which kernel:
      (254, 1280) lower-case: offered to the byte tile (left there) under every setting;
      (255, 1280) and (254, 1281) lower-case: offered to the wide kernel only -- counted by default, never with
                  DELLYHIP_SR_WIDE=0 (the byte tile did not take them);
      (319, 2049) lower-case: the strip kernel, offered to neither;
      clean (254, 1280) / (253, 1280) / (255, 1280) / (254, 1281) / (319, 2048): finished by the byte tile or the wide kernel (0 left)."""
    p = wide_params()
    b = R.counter_batch()
    rr, rb = reference.refine_batch(b, params=p, want_alignment=True, n_threads=THREADS)
    clean = np.array([t["noise"] == "clean" for t in b.truth])
    assert rr["ok"][clean].all()
    for name, env, left in (("default", {}, 3 + 4 + 5), ("nowide", {"DELLYHIP_SR_WIDE": "0"}, 3)):
        ctx = context(p, env)
        try:
            ctx.set_chromosomes(b.chroms)
            rbatch = ctx.upload(b)
            rbatch.run()
            assert rbatch.sparse_left() == left, name
            gr, gb = rbatch.fetch()
            rbatch.free()
        finally:
            ctx.close()
        compare(gr, gb, rr, rb, fields=_fields(False), blobs=_blobs(False), label="counters " + name)
    for name, keep, left in (("clean only", clean, 0), ("byte-tile lower-case only", ~clean & (np.array([t["m"] for t in b.truth]) == 254)
                                                         & (np.array([t["n"] for t in b.truth]) == 1280), 3)):
        sub = synth.subset(b, np.nonzero(keep)[0])
        ctx = context(p, {})
        try:
            ctx.set_chromosomes(sub.chroms)
            rbatch = ctx.upload(sub)
            rbatch.run()
            assert rbatch.sparse_left() == left, name
            rbatch.free()
        finally:
            ctx.close()


# ---- the hand-off to split_align_kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [False, True])
def test_deferred_wide_alphabet_seats(reference, port, want):
    """consensus strings of 15, 16, 17 and 60 distinct bytes (ACGT + upper / lower IUPAC, punctuation, bytes >= 0x80), written
    into the genome as well, each seated with three ordinary partners of its shape, at m = 31, 63, 95, 127, 159 (quad bins 1 .. 5;
    pair bins 1 .. 3 with DELLYHIP_QUAD=0 or as pair items under DELLYHIP_QUAD_MIX) and 191, 254, 318 (pair bins 3 .. 5).
    15 bytes stay in the packed kernels, 16 and more defer the whole wavefront (cntmax > 15, split_pk.hpp / split_quad.hpp) to
    split_align_kernel<K>; the deferred junction and its partners must all be the reference's.  (Such a consensus never leaves
    longNeedle with a split: the reference's reverseComplement keeps bytes it does not know in place, so its two DP passes
    disagree (src/needle.h:85) -- the records carry score_unsplit and the partners' splits.)
    The quad kernel's other deferral, a seat whose real m / n exceed the host's bound (split_quad.hpp:227), is not reachable
    through the C-ABI: every batch that gets quad seats has its window lengths computed exactly on the host (host_window_len,
    the same integer arithmetic as the window builder) and its consensus lengths known, and direct batches get no quad seats."""
    b = R.deferral_batch()
    p = abi.params_sr()
    (rr, _), _ = expected(reference, port, "defer", b, p)
    partner = np.array([t["distinct"] is None for t in b.truth])
    assert int(rr["ok"][partner].sum()) >= partner.sum() * 3 // 4
    for name, env in KNOBS.items():
        check_all(reference, port, "defer %s aln=%d" % (name, want), b, p, gpu_refine(b, p, env, want), want)


# ---- seat filling -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad_count,pair_count", [(5, 3), (6, 5), (7, 7)])
def test_partial_seats_and_unequal_partners(reference, port, quad_count, pair_count):
    """quad bins holding 5, 6, 7 junctions (1, 2, 3 mod 4: the last wavefront has 3, 2, 1 empty seats) and pair-only bins
    holding 3, 5, 7 (one empty seat), partners at nB = nA, nB << nA and nB <= 3 (a window clamped by a chromosome of 1 .. 3
    letters): every record is the reference's, and each junction's record is the one it gets when it is refined alone"""
    b = R.seat_batch(quad_count, pair_count)
    p = wide_params()
    label = "seats %d/%d" % (quad_count, pair_count)
    for name in ("dense", "pair", "dense-quadmix"):
        ctx = context(p, KNOBS[name])
        try:
            ctx.set_chromosomes(b.chroms)
            gr, gb = ctx.refine(b, want_alignment=True)
            check_all(reference, port, label, b, p, (gr, gb), True)
            for k in range(b.n):
                ar, ab = ctx.refine(synth.subset(b, [k]), want_alignment=True)
                compare(ar, ab, gr[k:k + 1], gb, fields=CORE + INTERNAL, label="%s %s junction %d alone" % (label, name, k))
        finally:
            ctx.close()


# ---- the other entry paths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(GRID))
def test_grid_through_stream_and_resident_reruns(reference, port, group):
    """the pipelined dellyhip_stream (BINS_LAZY: only the sparse list is built at submit; what the sparse kernels leave is
    routed to the dense bins at collect, BINS_LEFTOVER), and a resident batch run twice"""
    b, p = GRID[group]
    ctx = refine.Context(params=p)
    try:
        ctx.set_chromosomes(b.chroms)
        st = refine.Stream(ctx, depth=2)
        try:
            st.submit(b, tag=1)
            st.submit(b, tag=2)
            for tag in (1, 2):
                gr, gb, t = st.collect()
                assert t == tag
                check_all(reference, port, "grid %s stream %d" % (group, tag), b, p, (gr, gb), False)
        finally:
            st.close()
        rbatch = ctx.upload(b)
        try:
            for rep in range(2):
                rbatch.run()
                check_all(reference, port, "grid %s resident run %d" % (group, rep), b, p, rbatch.fetch(), False)
        finally:
            rbatch.free()
    finally:
        ctx.close()


def test_grid_through_single_item_long_needle(reference, gpu_ctx):
    """dellyhip_long_needle (the direct path: no sparse or quad route; the strip kernel beyond the short-read shapes) on one clean
    junction of every grid cell, consensus against its contiguous window"""
    cells = [(m, n, "del", "clean", 1) for m in R.GRID_M for n in R.GRID_N] + [(320, 1280, "del", "clean", 1), (330, 2100, "del", "clean", 1)]
    b = R.make(cells, seed=77)
    found = 0
    for k, (cons, win) in enumerate(R.windows(b)):
        assert len(cons) == b.truth[k]["m"] and len(win) == b.truth[k]["n"]
        rf, r0, r1, _ = reference.long_needle(cons, win)
        gf, g0, g1 = gpu_ctx.long_needle(cons, win)
        assert (gf, g0, g1) == (rf, r0 if rf else b"", r1 if rf else b""), b.truth[k]
        found += rf
    assert found >= len(cells) * 3 // 4


def test_wide_kernel_scratch_grows_on_one_context(reference):
    """launch_sparse_wide sizes its per-block tables from the list (32 blocks for a handful of junctions) and grows them behind a
    device synchronisation: a few wide-kernel junctions, then 1500 on the same context"""
    p = wide_params()
    ctx = refine.Context(params=p)
    try:
        for n, seed in ((5, 41), (1500, 42)):
            b = R.wide_kernel_batch(n, seed=seed)
            rr, rb = reference.refine_batch(b, params=p, want_alignment=False, n_threads=THREADS)
            assert int(rr["ok"].sum()) >= n * 3 // 4
            ctx.set_chromosomes(b.chroms)
            gr, gb = ctx.refine(b)
            compare(gr, gb, rr, rb, fields=_fields(False), blobs=_blobs(False), label="wide kernel x %d" % n)
    finally:
        ctx.close()
