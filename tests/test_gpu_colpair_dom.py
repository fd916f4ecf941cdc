"""Add+dom column-pair rounds (engine option f4_nc2_dom): items (I, J, 2) of two neighbouring column blocks in the
one-wave 32 x 64 instantiation of band_f4_kernel, in whole rounds; the pairs past the last full round go back to
single-block items and run, with the odd runs' leftover singles, in the single-block kernel.

Every case is one engine, one resident image, the same add+dom run with f4_nc2_dom 1 and then 0: the seven result
arrays bitwise equal (each (block pair, SNP) contribution is formed by the same pair_epilogue call on the same exact
integer Gram tile and added as a fixed-point integer) and flop_issued equal.  One case per family is also held to
the C oracle (default flags) or the fp64 truth (FLAG_EXACT_RARE) with the suite's bars (conftest.assert_ld_close).

Under super-item routing (missing-free blocks) both lists are compacted by the routing map and a pair may run with one
block.  Production runs take pair rounds only on long rows (N >= 2^17) with at least two rounds of 4 pairs per CU; the option
colpair_round_items sets the pairs per round for these shapes (N = 67: one chunk pair; N = 1 003), so the same
kernels, plan split, expansion and launch shaping run on a few dozen items (the production gate itself, 1 024-chunk
rows and saturated entries: test_gpu_colpair_long.py, test_gpu_saturation.py; production SNP counts:
test_gpu_schedule_scale.py; the *_case builders here are theirs too).  Which structures a case holds is
asserted from the host planner's paired plan (nldsc_plan_band, max_nc 2: the same runs of neighbouring column blocks,
paired from each row's first needed block) and from what the engine reports (band kernel, block pairs per round)."""
import numpy as np
import pytest

from conftest import assert_ld_close, rare_variant_set, record
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F4 = 16  # _lib.FLAG_EXACT_F4 (the other flags are read from _lib: flag())
KEYS = ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")


@pytest.fixture(scope="module", autouse=True)
def hip_runtime():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)


def flag(name):
    from nldsc_amd import _lib
    return getattr(_lib, name)


def geno(N, M, seed, missing):
    from nldsc_amd import synth
    return synth.genotypes(synth.SynthSpec(n_org=N, n_snp=M, length_cm=0.01 * M, seed=seed, missing=missing, rho=0.9))


def pack(g):
    from nldsc_amd import synth
    rows = synth.pack_bed_rows(g)
    return rows, synth.bed_bytes(rows)


def paired_plan(pos, wind, own=None):
    """The host planner's paired items [k, 4] = (I, J, z, 0) for all-pass flags."""
    from nldsc_amd import _lib
    return _lib.plan_band(pos, np.ones(len(pos), np.uint8), wind, own=own, max_nc=2)[2]


def structure(items):
    """Needed column blocks per row block, and the item forms."""
    need = {}
    for I, J, z, _ in items:
        need[int(I)] = need.get(int(I), 0) + int(z)
    return dict(need=set(need.values()), diag_pair=any(I == J and z == 2 for I, J, z, _ in items),
                pairs=int((items[:, 2] == 2).sum()), singles=int((items[:, 2] == 1).sum()))


def ab(bed, M, N, args, *, flags, round_items, options=None, own=None, want="f4_colpair", runner=None):
    """The run with f4_nc2_dom 1, then 0, on one engine: bitwise equal, flop_issued equal; returns (got, timings of
    the pair run)."""
    from nldsc_amd.engine import Engine
    opts = dict(options or {})
    if round_items:
        opts["colpair_round_items"] = round_items
    run = runner or (lambda e: e.run(*args, flags=flags, own=own))
    with Engine(0, options=opts) as e:
        e.load_bed_bytes(bed, M, N)
        e.set_option("f4_nc2_dom", 1)
        got = run(e)
        t1 = e.timings()
        e.set_option("f4_nc2_dom", 0)
        ref = run(e)
        t0 = e.timings()
    assert t0["band_kernel"] != "f4_colpair", t0
    if want == "f4_colpair":
        assert t1["band_kernel"] == "f4_colpair" and t1["band_round_items"] == 2 * round_items and t1["ksplit"] == 1, t1
    else:
        assert t1["band_kernel"] in want and t1["band_kernel"] == t0["band_kernel"], (t1, t0)
    assert t1["band_items"] == t0["band_items"], (t1["band_items"], t0["band_items"])
    assert t1["flop_issued"] == t0["flop_issued"], (t1["flop_issued"], t0["flop_issued"])
    for k in got:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    return got, t1


_sets: dict = {}


def base_set(N, M):
    """1 % missing in every block, 100 SNPs per window unit; (rows, bed, positions, arguments)."""
    if (N, M) not in _sets:
        rows, bed = pack(geno(N, M, seed=N + M, missing=0.01))
        pos = 0.01 * np.arange(M)
        _sets[N, M] = (rows, bed, pos)
    return _sets[N, M]


SHAPES = [
    # (N, M, window, pairs per round): 0.5 = 50 SNPs reach two blocks ahead (rows of 3, 2 and 1 needed blocks);
    # M = 32 k + 1: a last block of one SNP
    (67, 33, 0.5, 1),      # one pair item, the diagonal pair (0, 0)+(0, 1), and the one-SNP block's single
    (67, 225, 0.5, 4),     # 8 blocks: 7 pairs (one full round of 4, 3 back to singles) and the leftover singles
    (1003, 225, 0.5, 2),
    (1003, 385, 0.2, 3),   # 13 blocks, 20 SNPs reach one block ahead: every row one pair, the last row a single
    (1003, 400, 0.9, 5),   # rows of 4 needed blocks: two pairs each
]


@pytest.mark.parametrize("N,M,wind,round_items", SHAPES)
def test_pair_rounds_bitwise_single_blocks(N, M, wind, round_items):
    rows, bed, pos = base_set(N, M)
    st = structure(paired_plan(pos, wind))
    assert st["diag_pair"] and st["pairs"] >= round_items, st
    if (M, wind) == (225, 0.5):
        assert {1, 2, 3} <= st["need"] and st["singles"] >= 2 and st["pairs"] % round_items, st
    if M % 32 == 1:
        assert (M + 31) // 32 - 1 in {int(j) + int(z) - 1 for _, j, z, _ in paired_plan(pos, wind)}
    args = (wind, 0.0, 1e-5, 0.01, pos)
    got, t = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items)
    if (N, M) == (1003, 225):
        exp = O.run_f64(rows, N, *args)
        assert_ld_close(got, exp, tol=dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12), residuals_std=(1e-12, 1e-10),
                                           maf=(0.0, 0.0)), label="colpair vs fp64 truth")
    record(f"colpair_dom_n{N}_m{M}", dict(round_items=round_items, tail_ksplit=t["band_tail_ksplit"], **{
        k: v for k, v in st.items() if k != "need"}))


def missing_in_blocks(N, M, blocks, seed):
    """Missing-free genotypes with 20 missing calls in one SNP of each listed 32-SNP block."""
    g = geno(N, M, seed=seed, missing=0.0)
    rng = np.random.default_rng(seed)
    for b in blocks:
        j = 32 * b + int(rng.integers(0, min(32, M - 32 * b)))
        g[j, rng.choice(N, 20, replace=False)] = -1
    return g


def missing_patterns_case(N):
    """Blocks 0 and 5 of 8 hold missing calls and the window reaches three blocks ahead (two pair items per row);
    asserts that all four (row, columns) missingness patterns occur among the pair items.  Returns (rows, bed, M, run
    arguments, pairs per round, options)."""
    from test_gpu_parity import missing_free_blocks
    M, wind, miss = 225, 0.9, {0, 5}
    rows, bed = pack(missing_in_blocks(N, M, sorted(miss), seed=N))
    assert missing_free_blocks(rows, N) == 6
    pos = 0.01 * np.arange(M)
    items = paired_plan(pos, wind)
    pats = {(int(I) in miss, int(J) in miss or int(J) + 1 in miss) for I, J, z, _ in items if z == 2}
    assert pats == {(False, False), (False, True), (True, False), (True, True)}, pats
    assert any(z == 2 and (int(J) in miss) != (int(J) + 1 in miss) for _, J, z, _ in items)
    return rows, bed, M, (wind, 0.0, 1e-5, 0.01, pos), 3, {"t2": 0}


@pytest.mark.parametrize("N", [67, 1003])
def test_row_and_column_missing_patterns(N):
    """Blocks 0 and 5 of 8 hold missing calls and the window reaches three blocks ahead (two pair items per row): a
    pair item's loop follows its row block and the union of its two column blocks, and all four (row, columns)
    patterns occur — (0, 0)+(0, 1) and (4, 4)+(4, 5) with column blocks that differ in missingness.  Super-item
    routing off (t2 0): the missing-free blocks would otherwise send the run to the super-item kernels."""
    rows, bed, M, args, round_items, options = missing_patterns_case(N)
    got, _ = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items, options=options)
    if N == 1003:
        assert_ld_close(got, O.run_f64(rows, N, *args), tol=dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12),
                        residuals_std=(1e-12, 1e-10), maf=(0.0, 0.0)), label="colpair missing patterns")


def routed_map(M, miss, shift):
    """routed(I, J): the super-item of 2^shift blocks a side that holds block pair (I, J) is missing-free in its
    (clamped) row and column blocks, so a super-item kernel takes the pair (t2_routed / q_routed)."""
    nblk, F = (M + 31) // 32, 1 << shift

    def free(b):
        return not any(min(F * (b // F) + k, nblk - 1) in miss for k in range(F))
    return lambda I, J: free(int(I)) and free(int(J))


def routing_case(N, t2, shift):
    """Mostly missing-free data under super-item routing: blocks 4-7 of 13 hold missing calls, every other block is
    free; asserts from the paired plan and the blocks' missingness that pairs lose both, one and none of their blocks.
    Returns (rows, bed, M, run arguments, pairs per round, options, the counts recorded)."""
    M, wind, miss = 385, 0.9, {4, 5, 6, 7}
    rows, bed = pack(missing_in_blocks(N, M, sorted(miss), seed=11 + t2))
    pos = 0.01 * np.arange(M)
    routed = routed_map(M, miss, shift)
    pairs = [(int(I), int(J)) for I, J, z, _ in paired_plan(pos, wind) if z == 2]
    lost = [(routed(I, J), routed(I, J + 1)) for I, J in pairs]
    one = sum(a != b for a, b in lost)
    kept = sum(not (a and b) for a, b in lost)
    assert one >= 2 and any(a and b for a, b in lost) and any(not a and not b for a, b in lost), lost
    assert (1, 3) in pairs and routed(1, 3) and not routed(1, 4)
    round_items = 5
    assert kept >= round_items and kept % round_items, kept
    return (rows, bed, M, (wind, 0.0, 1e-5, 0.01, pos), round_items, {"ksplit": 0, "t2": t2},
            dict(pairs=len(pairs), kept=kept, lose_one_block=one))


@pytest.mark.parametrize("t2,shift", [(3, 2), (1, 1)], ids=["quad", "2x2"])
def test_routing_drops_one_block_of_a_pair(t2, shift):
    """Mostly missing-free data under super-item routing: blocks 4-7 of 13 hold missing calls, every other block is
    free.  The super-item kernel takes the missing-free super-items; of the pairs, those with both blocks routed
    leave the compacted pair list, those with none run whole, and the pairs that straddle a super-column edge —
    (1, 3)+(1, 4), (3, 3)+(3, 4): block 3 routed, block 4 not — lose exactly one block in the pair kernel (r0 / r1)
    and run the single-block body on the other.  The last pairs' expanded single blocks go through the routing map
    too.  Asserted from the paired plan and the blocks' missingness; bitwise option 0 (the routed single-block run)
    with flop_issued equal, and held to the fp64 truth."""
    N = 1003
    rows, bed, M, args, round_items, options, counts = routing_case(N, t2, shift)
    got, t = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items, options=options)
    assert_ld_close(got, O.run_f64(rows, N, *args), tol=dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12),
                    residuals_std=(1e-12, 1e-10), maf=(0.0, 0.0)), label="colpair under routing")
    record(f"colpair_dom_routed_t2_{t2}", counts)


def test_unfused_plan_chain():
    """The split plan behind the kernel chain of long slices (plan_fused 0: launch_plan, then the split), as
    production-size chromosomes run it."""
    N, M, wind = 1003, 400, 0.9
    rows, bed, pos = base_set(N, M)
    ab(bed, M, N, (wind, 0.0, 1e-5, 0.01, pos), flags=F4 | flag("FLAG_EXACT_RARE"), round_items=5,
       options={"plan_fused": 0})


def one_replayed_case(N):
    """One rare variant (8 hom-A2 and 60 het calls: replayed) in block 3 only; asserts that the pair (2, 2)+(2, 3) is
    planned.  Returns (bed, M, run arguments, pairs per round)."""
    from nldsc_amd import synth
    M, wind = 225, 0.5
    g = geno(N, M, seed=N + M, missing=0.01)
    rng = np.random.default_rng(21)
    pick = rng.choice(N, 68, replace=False)
    g[100] = 0
    g[100, pick[:60]], g[100, pick[60:]] = 1, 2
    rows = synth.pack_bed_rows(g)
    bed = synth.bed_bytes(rows)
    pos = 0.01 * np.arange(M)
    assert any(z == 2 and (int(I), int(J)) == (2, 2) for I, J, z, _ in paired_plan(pos, wind))
    return bed, M, (wind, 1e-4, 1e-5, 0.01, pos), 3


@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "kc_launch"])
def test_one_replayed_block_in_a_pair(defer):
    """One rare variant (8 hom-A2 and 60 het calls: replayed) in block 3 only: the pair (2, 2)+(2, 3) holds it in
    one of its three blocks, so its clean block pair (2, 2) goes through the deferred (or KC) epilogue with it, where
    option 0 runs (2, 2) in the main launch; (3, 3)+(3, 4) holds it in the row block."""
    N = 1003
    bed, M, args, round_items = one_replayed_case(N)
    got, _ = ab(bed, M, N, args, flags=F4, round_items=round_items, options={"defer_rep": defer})
    if defer:
        assert_ld_close(got, O.run_c(bed, M, N, *args), label="colpair, one replayed block vs oracle")


@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "kc_launch"])
def test_replayed_rare_variants_inside_pair_items(defer):
    """Default flags: every other SNP is a rare variant whose fp32 residual is replayed, so every pair item holds
    one: their K loops run in the pair launch with the Gram tiles kept for the deferred epilogue (defer_rep 1), or
    the items wait for the KC instantiation of the one-wave kernel (defer_rep 0)."""
    N, M, wind = 1003, 200, 1.0
    rows, pos = rare_variant_set(N, n_snp=M)
    from nldsc_amd import synth
    bed = synth.bed_bytes(rows)
    st = structure(paired_plan(pos, wind))
    assert st["pairs"] >= 4 and st["diag_pair"], st
    args = (wind, 1e-5, 1e-5, 1.0 / M, pos)
    got, _ = ab(bed, M, N, args, flags=F4, round_items=4, options={"defer_rep": defer})
    if defer:
        assert_ld_close(got, O.run_c(bed, M, N, *args), label="colpair, replayed rare variants vs oracle")


def test_owned_range_cuts_through_a_pair():
    """own = [40, 150) of 225: block 1 is partly owned on the left (rows of block 0 reach it), block 4 partly on the
    right; pair items straddle both edges."""
    N, M, wind = 1003, 225, 0.5
    rows, bed, pos = base_set(N, M)
    own = (40, 150)
    items = paired_plan(pos, wind, own=own)
    assert any(z == 2 and 32 * J < own[1] < 32 * (J + 2) for _, J, z, _ in items), items
    assert any(z == 2 and 32 * I < own[0] < 32 * (I + 1) for I, _, z, _ in items), items
    args = (wind, 0.0, 1e-5, 0.01, pos)
    got, _ = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=2, own=own)
    exp = O.run_f64(rows, N, *args)
    sub = {k: got[k][own[0]:own[1]] for k in KEYS}
    assert_ld_close(sub, {k: exp[k][own[0]:own[1]] for k in KEYS},
                    tol=dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12), residuals_std=(1e-12, 1e-10), maf=(0.0, 0.0)),
                    label="colpair owned range")


@pytest.mark.parametrize("round_items", [0, 64], ids=["production_round", "round_above_the_pairs"])
def test_below_one_round_runs_the_single_block_plan(round_items):
    """Fewer pairs than one round (the production round of 4 per CU on short rows, or a 64-pair round against 7
    pairs): no pair item runs, and the run reports the K-split or the single-block kernel as before."""
    N, M, wind = 1003, 225, 0.5
    rows, bed, pos = base_set(N, M)
    ab(bed, M, N, (wind, 0.0, 1e-5, 0.01, pos), flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items,
       want=("f4", "f4_ksplit"))


@pytest.mark.parametrize("kind", ["annot", "pairs", "covar"])
def test_annot_pairs_covar_take_no_pair_items(kind):
    """Annotated, pair-table and covariate runs keep their batches of single-block items."""
    N, M, wind = 1003, 225, 0.5
    rows, bed, pos = base_set(N, M)
    args = (wind, 0.0, 1e-5, 0.01, pos)
    rng = np.random.default_rng(3)
    if kind == "annot":
        a = np.stack([np.ones(M), (np.arange(M) % 3 == 0).astype(float), rng.standard_normal(M)], axis=1)
        runner = lambda e: e.run(*args, flags=F4, annot=a)  # noqa: E731
    elif kind == "pairs":
        def runner(e):
            t = e.run_pairs(*args, flags=F4)
            return {k: np.asarray(v) for k, v in t.items() if k != "n_pairs"}
    else:
        c = rng.standard_normal((N, 3))
        q, _ = np.linalg.qr(c - c.mean(0))
        runner = lambda e: e.run(*args, flags=F4, covar=q)  # noqa: E731
    ab(bed, M, N, args, flags=F4, round_items=2, want=("f4", "f4_ksplit"), runner=runner)
