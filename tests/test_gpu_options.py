"""-m gpu: the refinement path under non-default `delly sr` / `delly lr` options, against the reference itself (oracle/_ref).

dellyhip_params is not a constant in Delly: `delly lr` takes -w minConsWindow, -f minimumFlankSize, -a flankQuality,
-i indelsize and -z minCliqueSize (src/tegua.h:230-241), `delly sr` -z and -w (src/delly.h:221,240).  Every other GPU test
runs the long-read kernels at params_lr() and the short-read MSA at minCliqueSize 2, where min(minCliqueSize, rows) never
matters.  Here each option is changed on its own, and the junctions are built so that the comparisons the options feed sit
exactly on their thresholds (tests/fuzz.py at_span / ins_at_flank, and values read back from the reference's own records):
  svEnd - svStart <= indelsize, > minConsWindow      (src/split.h:116,124,139,158,606)
  consensus.size() < 2 * minimumFlankSize + insLen    (src/split.h:647)
  bufferSpace = max((m - insLen) / 3, minimumFlankSize)  (src/split.h:652)
  percId < flankQuality, the flank tests              (src/split.h:364,370-371)
  cov >= max(2, min(minCliqueSize, rows))             (src/msa.h:135)
Every CORE field, the consensus and allele bytes, and (where requested) the alignment rows must equal the reference's."""
import os

import numpy as np
import pytest

import fuzz
from delly_amd import abi, refine, synth
from util import CORE, compare

pytestmark = pytest.mark.gpu
THREADS = min(os.cpu_count() or 1, 64)


def params(base, **kw):
    p = abi.params_lr(realign=True) if base == "lr" else abi.params_sr()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gpu_refine(batch, p, want_alignment, env=None):
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = refine.Context(params=p)   # (the knobs are read at dellyhip_create)
        try:
            ctx.set_chromosomes(batch.chroms)
            return ctx.refine(batch, want_alignment=want_alignment)
        finally:
            ctx.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check(reference, batch, p, label, wants=(False, True), env=None, min_ok=0, ref=None):
    """HIP against the reference with and without alignment rows -> the reference's (records, blob)"""
    rr, rb = ref if ref is not None else reference.refine_batch(batch, params=p, want_alignment=True, n_threads=THREADS)
    assert int(rr["ok"].sum()) >= min_ok, (label, int(rr["ok"].sum()), min_ok)
    for want in wants:
        gr, gb = gpu_refine(batch, p, want, env)
        compare(gr, gb, rr, rb, fields=[f for f in CORE if want or f != "aln_len"],
                blobs=("cons", "allele", "aln") if want else ("cons", "allele"), label="%s aln=%d" % (label, want))
    return rr, rb


# ---- 1. the long-read option grid -------------------------------------------------------------------------------------
LR_GRID = [("minimum_flank_size", 30), ("minimum_flank_size", 250), ("flank_quality", 0.8), ("flank_quality", 0.97),
           ("indelsize", 500), ("indelsize", 30000), ("min_cons_window", 300), ("min_cons_window", 3000)]
LR_BATCHES = {   # (mode, n_reads): (junctions, least number of accepted junctions at any grid point)
    ("lr", 0): (12, 6), ("lrins", 0): (8, 4), ("lr", 4): (6, 3), ("lrins", 4): (6, 3)}


def lr_batch(mode, n_reads):
    n = LR_BATCHES[(mode, n_reads)][0]
    return synth.make_batch(n, seed=301 + n_reads, mode=mode, n_reads=n_reads, sub_rate=0.04 if n_reads else 0.01)


@pytest.mark.parametrize("mode,n_reads", list(LR_BATCHES), ids=lambda x: str(x))
@pytest.mark.parametrize("option,value", LR_GRID, ids=lambda x: str(x))
def test_long_read_option_grid(reference, option, value, mode, n_reads):
    """lr_kernel / lrins_kernel (n_reads 0), msaEdlib (lr) and msaWfa (lrins, whose anchors are minConsWindow bases of
    reference, src/assemble.h:855-856) + alignConsensus(realign) with one `delly lr` option changed"""
    p = params("lr", **{option: value})
    check(reference, lr_batch(mode, n_reads), p, "%s=%s %s/%d" % (option, value, mode, n_reads),
          min_ok=LR_BATCHES[(mode, n_reads)][1])


# ---- 2. long alleles under a large -i --------------------------------------------------------------------------------
BIG_SHAPES = [(1000, 10500), (900, 16000), (800, 22000), (700, 28000), (1200, 20000)]   # (flank, DEL length): window 2 m + ell < LR_NMAX


def test_long_alleles_under_large_indelsize(reference):
    """deletions of 10 .. 28 kb under -i 30000: one contiguous window of up to ~31 000 columns and a REF allele of the whole
    deletion (src/split.h:116,606) -- through the host-buffer call (slots sized in batch_upload) and a resident batch"""
    p = params("lr", indelsize=30000)
    b = synth.make_big_deletions(BIG_SHAPES, seed=5)
    rr, rb = check(reference, b, p, "big DEL -i 30000", min_ok=len(BIG_SHAPES))
    assert rr["allele_len"].min() > 10000 and rr["allele_len"].max() > 28000
    ctx = refine.Context(params=p)
    try:
        ctx.set_chromosomes(b.chroms)
        rbatch = ctx.upload(b)
        rbatch.run()
        gr, gb = rbatch.fetch()
        rbatch.free()
    finally:
        ctx.close()
    compare(gr, gb, rr, rb, fields=[f for f in CORE if f != "aln_len"], blobs=("cons", "allele"), label="big DEL resident")


def test_long_alleles_through_msa_edlib_under_large_indelsize(reference):
    """the same through msaEdlib: the long-read MSA batch sizes its allele slots from indelsize (acap + min(LR_NMAX, 2 acap
    + indelsize)); a slot sized for -i 10000 cannot hold these REF alleles"""
    p = params("lr", indelsize=30000)
    b = synth.make_big_deletions([(1000, 24000), (1000, 14000), (800, 27000)], seed=12, n_reads=4)
    rr, _ = check(reference, b, p, "big DEL msaEdlib -i 30000", min_ok=3)
    assert rr["allele_len"].max() > 27000


def test_window_beyond_lr_nmax_is_a_flagged_limit(reference):
    """a contiguous window of 2 m + ell > LR_NMAX (32 000) columns: E_LIMIT and ok == 0, never a silently wrong record; the
    junctions beside it are the reference's"""
    p = params("lr", indelsize=30000)
    b = synth.make_big_deletions([(1000, 20000), (1500, 29500), (900, 12000)], seed=13)
    rr, rb = reference.refine_batch(b, params=p, want_alignment=True, n_threads=THREADS)
    assert int(rr["ref_len"][1]) > 32000 and int(rr["ok"][1]) == 1
    for want in (False, True):
        gr, gb = gpu_refine(b, p, want)
        assert int(gr["status"][1]) == abi.E_LIMIT and int(gr["ok"][1]) == 0, gr[["status", "ok"]]
        keep = np.array([0, 2])
        compare(gr[keep], gb, rr[keep], rb, fields=[f for f in CORE if want or f != "aln_len"],
                blobs=("cons", "allele", "aln") if want else ("cons", "allele"), label="beside the limit aln=%d" % want)
        assert int(gr["ok"][keep].sum()) == 2


# ---- 3. the consensus threshold -z on the short-read MSA ----------------------------------------------------------------
MSA_ROUTES = {"default": ({}, 150), "team2": ({"DELLYHIP_MSA_TEAM": "2"}, 150), "team4": ({"DELLYHIP_MSA_TEAM": "4"}, 150),
              "direct_float": ({"DELLYHIP_MSA_TMAX": "0"}, 150), "msa_big": ({}, 250)}
MSA_READS = [2, 3, 7, 20, (2, 9)]
_MSA_REF = {}


def msa_batch(n_reads, read_len):
    n = 12 if read_len > 150 else 24
    return synth.make_batch(n, mode="c2", seed=311, n_reads=n_reads, read_len=read_len, cons_flank=read_len, sub_rate=0.02)


@pytest.mark.parametrize("route", list(MSA_ROUTES))
@pytest.mark.parametrize("z", [3, 5, 20])
def test_msa_min_clique_size(reference, z, route):
    """cov >= max(2, min(minCliqueSize, rows)) in the consensus of every MSA instance: the single wavefront, the team of 2
    and 4 wavefronts, the direct-float kernel and msa_big (250 bp reads)"""
    env, read_len = MSA_ROUTES[route]
    p = params("sr", min_clique_size=z)
    for nr in MSA_READS:
        b = msa_batch(nr, read_len)
        key = (z, str(nr), read_len)
        if key not in _MSA_REF:
            _MSA_REF[key] = reference.refine_batch(b, params=p, want_alignment=True, n_threads=THREADS)
        check(reference, b, p, "-z %d %s reads %s" % (z, route, nr), wants=(False,) if route != "default" else (False, True),
              env=env, min_ok=b.n // 3, ref=_MSA_REF[key])


@pytest.mark.parametrize("z", [3, 5, 20])
def test_msa_single_call_min_clique_size(reference, z):
    """the drop-in msa(): Context(params).msa(reads) against the reference's msa() at the same parameters"""
    p = params("sr", min_clique_size=z)
    b = msa_batch((3, 12), 150)
    old = reference.params
    reference.params = p
    ctx = refine.Context(params=p)
    try:
        for k in range(8):
            reads = b.seqs_of(k)
            assert ctx.msa(reads) == reference.msa(reads), (z, k, len(reads))
    finally:
        ctx.close()
        reference.params = old


def test_long_read_msa_min_clique_size(reference):
    """msaEdlib ends in the same consensus() (src/assemble.h:461, src/msa.h:135): -z reaches the long-read MSA too (the
    lrmsa kernel's consensus_node).  At -z 5 and 20 the records differ from those at -z 3, and each is the reference's."""
    b = synth.make_batch(6, seed=321, mode="lr", n_reads=5, sub_rate=0.05)
    out = {}
    for z in (3, 5, 20):
        rr, _ = check(reference, b, params("lr", min_clique_size=z), "lr msa -z %d" % z, wants=(False,), min_ok=3)
        out[z] = rr
    assert (out[20]["cons_len"] != out[3]["cons_len"]).any()


# ---- 4. exact thresholds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,span,n", [("sr", 400, 48), ("sr", 1000, 48), ("lr", 3000, 24)])
def test_span_on_indelsize_and_min_cons_window(reference, base, span, n):
    """DEL / DUP / INV 3to3 / INV 5to5 reported with svEnd - svStart = T - 1, T, T + 1 at indelsize = minConsWindow = T:
    contiguous window or two, exact alleles or none (src/split.h:116,124,139,158,606)"""
    p = params(base, indelsize=span, min_cons_window=span)
    b = fuzz.at_span(n, span, seed=span, lr=base == "lr")
    rr, _ = check(reference, b, p, "span %s %d" % (base, span), min_ok=n * 3 // 4)
    d = b.junctions["sv_end"] - b.junctions["sv_start"] - span
    dels = (b.junctions["svt"] == 2) & (rr["ok"] != 0)
    assert ((rr["allele_len"][dels] > 0) == (d[dels] <= 0)).all() and (d[dels] == 0).any()


@pytest.mark.parametrize("base,mfs,span,n", [("sr", 40, 500, 24), ("sr", 60, 300, 24), ("lr", 500, 2000, 12)])
def test_consensus_length_on_twice_the_flank(reference, base, mfs, span, n):
    """|consensus| = 2 minimumFlankSize - 1, + 0, + 1 (src/split.h:647): only the first returns before it builds a window
    (ref_len 0); the others are aligned and then refused by the flank tests"""
    p = params(base, minimum_flank_size=mfs)
    b = fuzz.at_span(n, span, seed=mfs, lr=base == "lr", flank=mfs)
    rr, _ = check(reference, b, p, "|consensus| vs 2 * %d" % mfs)
    assert ((rr["ref_len"] > 0) == (rr["cons_len"] >= 2 * mfs)).all()
    assert (rr["cons_len"] == 2 * mfs).any() and (rr["cons_len"] == 2 * mfs - 1).any()


@pytest.mark.parametrize("buffer", [False, True])
@pytest.mark.parametrize("base,mfs,n", [("sr", 40, 30), ("lr", 300, 10)])
def test_insertion_flank_thresholds(reference, base, mfs, n, buffer):
    """svt 4: |consensus| = 2 minimumFlankSize + insLen + (1, 0, -1), and (|consensus| - insLen) / 3 around
    minimumFlankSize, where it takes over bufferSpace and so the width of the reference window (src/split.h:647-653)"""
    p = params(base, minimum_flank_size=mfs)
    b = fuzz.ins_at_flank(n, mfs, seed=mfs + buffer, lr=base == "lr", buffer=buffer)
    rr, _ = check(reference, b, p, "ins %s mfs %d buffer=%d" % (base, mfs, buffer))
    thr = 2 * mfs + b.junctions["ins_len"]
    assert ((rr["ref_len"] > 0) == (rr["cons_len"] >= thr)).all()
    if buffer:
        assert len(set(rr["ref_len"].tolist())) >= 3   # bufferSpace mfs - 1 -> mfs, mfs, mfs + 1: the window widths differ
    else:
        assert (rr["cons_len"] == thr).any() and (rr["cons_len"] == thr - 1).any()


def _at_value(reference, b, p_of, values, label):
    out = []
    for v in values:
        p = p_of(v)
        rr, _ = check(reference, b, p, "%s %r" % (label, v))
        out.append(rr)
    return out


@pytest.mark.parametrize("base,span,n", [("sr", 400, 24), ("lr", 3000, 12)])
def test_flank_tests_at_the_slack(reference, base, span, n):
    """minimumFlankSize = the largest value a junction's flank tests pass (src/split.h:370-371), and one more"""
    b = fuzz.at_span(n, span, seed=7 + span, lr=base == "lr")
    rr, _ = reference.refine_batch(b, params=params(base), want_alignment=False, n_threads=THREADS)
    slack = fuzz.flank_slack(rr)
    for s in sorted(set(slack[slack > 0].tolist()))[:2]:
        at, above = _at_value(reference, b, lambda v: params(base, minimum_flank_size=v), (s, s + 1), "flank %s" % base)
        hit = slack == s
        assert (at["ok"][hit] != 0).all() and (above["ok"][hit] == 0).all(), (s, at["ok"][hit], above["ok"][hit])


@pytest.mark.parametrize("base,span,n", [("sr", 400, 24), ("lr", 3000, 12)])
def test_flank_quality_at_a_reported_quality(reference, base, span, n):
    """flankQuality = exactly a srAlignQuality the reference reports (float32), and the next float above: the junction is
    accepted at the value and refused above it (percId < flankQuality, src/split.h:364)"""
    b = fuzz.at_span(n, span, seed=11 + span, lr=base == "lr")
    rr, _ = reference.refine_batch(b, params=params(base, flank_quality=0.0), want_alignment=False, n_threads=THREADS)
    q = rr["sr_align_quality"][(rr["ok"] != 0) & (rr["sr_align_quality"] < 1)]
    assert q.size >= 2
    for v in (np.float32(q.min()), np.float32(np.median(q))):
        v = q[np.argmin(np.abs(q - v))]
        up = np.nextafter(v, np.float32(2))
        at, above = _at_value(reference, b, lambda x: params(base, flank_quality=float(x)), (v, up), "flank quality %s" % base)
        hit = (rr["ok"] != 0) & (rr["sr_align_quality"] == v)
        assert hit.any() and (at["ok"][hit] != 0).all() and (above["ok"][hit] == 0).all(), (float(v), at["ok"][hit], above["ok"][hit])


# ---- 5. scoring at the guard of the packed two-merges-per-pass route -------------------------------------------------------
@pytest.mark.parametrize("score", [(30, -30, -16, -15), (31, -4, -10, -1)], ids=["inside", "outside"])
def test_msa_scoring_at_the_packed_guard(reference, score):
    """pair_params_ok (msa_body.inc): packed int16 merges inside the guard, one merge at a time outside it"""
    p = abi.Params(*score, 2, 13, 1000, 100, 0.95, 0)
    b = synth.make_batch(24, mode="c2", seed=331, n_reads=(3, 9), sub_rate=0.02)
    check(reference, b, p, "scoring %s" % (score,), min_ok=6)
