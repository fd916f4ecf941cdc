"""Add+dom column-pair rounds through the production gate, with no test option: rows of n_it >= 1024 chunks
(N >= 2^17 - 255), at least COLPAIR_ROUND_MIN = 2 rounds of 4 pairs per CU, the round 4 n_cu (ld_engine.cpp
schedule_on_gpu / enqueue_band, band_plan.cpp shape_colpair), on the smallest band that passes it on the device at
hand — and the same band one row chunk pair shorter and one block smaller, where no pair item may run.

The band: nb blocks, nb the smallest count with sum_{n=1..nb} floor(n / 2) >= 8 n_cu pairs and nb (nb + 1) / 2 >=
16 n_cu block pairs (256 CUs: nb = 91, 2 070 pairs, 4 186 items; nb = 90 fails both with 2 025 and 4 095), M =
32 (nb - 1) + 1 SNPs (a last block of one SNP) in one window.  The rows are 97 distinct ones (test_gpu_schedule_scale
fast_genotypes, 1 % missing calls) repeated on the packed rows: 97 is coprime to 32, so no two blocks have the same
composition, and every SNP's scores follow from the 97 rows' exact pairs by multiplicity (test_gpu_saturation
multiplicity_truth).  The lists the engine reports (nldsc_engine_band_pair_items) are held to the restated schedule
(test_gpu_schedule_scale schedule_restated).

The all-missing rows reach one instantiation of the pair loop; the others — mixed row / column missingness, pairs that
lose a block to the routing, pair items with a replayed SNP — rerun the cases of test_gpu_colpair_dom.py at N = 2^17 - 1
(1 024 chunks) with the round option those tests set, against the fp64 truth at SNPs at both ends of every block (the
full truth takes half a minute at this N) or the C oracle.
"""
import numpy as np
import pytest

from conftest import assert_ld_close
from oracle import oracle as O
from test_gpu_colpair_dom import F4, ab, flag, missing_patterns_case, one_replayed_case, routing_case
from test_gpu_saturation import (LD_WIND, STD_THR, THREADS, check_multiplicity, exact_pairs, exact_r2d, bitwise,
                                 multiplicity_truth)
from test_gpu_schedule_scale import fast_genotypes, schedule_restated

N_GATE = (1 << 17) - 129   # 1 023 chunks, padded to n_it = 1 024: a 127-sample chunk and an all-padding one
N_BELOW = (1 << 17) - 256  # n_it = 1 022
DISTINCT = 97
EXACT = dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12), residuals_std=(1e-12, 1e-10), maf=(0.0, 0.0))


@pytest.fixture(scope="module")
def hip_runtime():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    yield
    _rows.clear()


def gpu(test):
    return pytest.mark.gpu(pytest.mark.usefixtures("hip_runtime")(test))


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def gate_blocks(n_cu):
    """The smallest block count whose band holds two rounds of 4 pairs per CU and twice that in block pairs."""
    nb = 1
    while sum(n // 2 for n in range(1, nb + 1)) < 8 * n_cu or nb * (nb + 1) // 2 < 16 * n_cu:
        nb += 1
    return nb


def test_gate_blocks_at_256_cus():
    assert gate_blocks(256) == 91
    assert (sum(n // 2 for n in range(1, 92)), 91 * 92 // 2) == (2070, 4186)
    assert (sum(n // 2 for n in range(1, 91)), 90 * 91 // 2) == (2025, 4095)


_rows: dict = {}


def distinct_rows(N):
    """(packed rows [97][bytes], exact pairs, rsq_thr, the 97 rows' own truth) at the first N samples of one draw."""
    from nldsc_amd import synth
    if N not in _rows:
        g = fast_genotypes(DISTINCT, N_GATE, seed=2024, missing=0.01)[:, :N]
        rows = synth.pack_bed_rows(np.ascontiguousarray(g))
        O.code_counts(synth.bed_bytes(rows), DISTINCT, N, threads=THREADS)  # (sets the oracle's OpenMP team size)
        po = exact_pairs(rows, N)
        r2d = exact_r2d(po)
        # independent residuals at this N: the exact r2d lie within a few 1e-4 of 0, thousands of them within 1e-5, so
        # the threshold goes into their upper tail, the first value there clear of every one of them
        rsq = next(c for c in np.quantile(r2d, 0.95) + 1e-6 * np.arange(1000) if np.abs(r2d - c).min() > 1.5e-6)
        assert np.abs(r2d - rsq).min() > 1e-6 and (r2d > rsq).sum() >= 5
        per_snp = O.run_f64_targets(rows, N, LD_WIND, 0.0, STD_THR, rsq, np.arange(DISTINCT) * 0.01,
                                    np.arange(DISTINCT))
        assert np.isfinite(per_snp["residuals_std"]).all()
        _rows[N] = (rows, po, float(rsq), per_snp)
    return _rows[N]


def band(N, M):
    """(bed image, positions, rsq_thr, truth) of M SNPs repeating the distinct rows, one window."""
    from nldsc_amd import synth
    rows, po, rsq, per_snp = distinct_rows(N)
    big = synth.bed_bytes(np.tile(rows, (M // DISTINCT + 1, 1))[:M])
    pos = np.arange(M, dtype=np.float64) * 1e-4
    assert pos[-1] < LD_WIND
    return big, pos, rsq, multiplicity_truth(po, M, rsq, per_snp)


def pair_lists(t):
    return t["band_pair_items"], t["band_pairs"], t["band_pair_rest"]


def run_on_off(bed, M, N, pos, rsq):
    """Default options, then f4_nc2_dom 0 on the same engine: ((results, timings), (results, timings))."""
    from nldsc_amd.engine import Engine
    out = []
    with Engine(0) as e:
        e.load_bed_bytes(bed, M, N)
        for on in (1, 0):
            if not on:
                e.set_option("f4_nc2_dom", 0)
            out.append((e.run(LD_WIND, 0.0, STD_THR, rsq, pos, flags=F4 | flag("FLAG_EXACT_RARE")), e.timings()))
    (a, ta), (b, tb) = out
    assert tb["band_kernel"] != "f4_colpair" and pair_lists(tb) == (0, 0, 0), tb
    assert ta["band_items"] == tb["band_items"] == (M + 31) // 32 * ((M + 31) // 32 + 1) // 2
    assert ta["flop_issued"] == tb["flop_issued"] > 0, (ta["flop_issued"], tb["flop_issued"])
    bitwise(a, b, "f4_nc2_dom 1 vs 0")
    return out


@gpu
def test_smallest_band_that_passes_the_gate():
    """n_it = 1 024 exactly and two rounds of pairs exactly reached: pair rounds by default, the lists the restated
    schedule's, every SNP's scores the truth by multiplicity, bitwise the single-block run."""
    n_cu = cu_count()
    nb = gate_blocks(n_cu)
    M, N = 32 * (nb - 1) + 1, N_GATE
    bed, pos, rsq, exp = band(N, M)
    (got, t), _ = run_on_off(bed, M, N, pos, rsq)
    s = schedule_restated(pos, LD_WIND)
    assert s["nblk"] == nb and s["items"] == nb * (nb + 1) // 2 and s["split_pairs"] >= 8 * n_cu
    assert t["band_kernel"] == "f4_colpair" and t["band_round_items"] == 8 * n_cu and t["ksplit"] == 1, t
    rnd = 4 * n_cu
    assert pair_lists(t) == (s["split_pairs"] // rnd * rnd, s["split_pairs"],
                             s["split_singles"] + 2 * (s["split_pairs"] % rnd)), (pair_lists(t), s["split_pairs"])
    if n_cu == 256:
        assert pair_lists(t) == (2048, 2070, 46 + 44)
    check_multiplicity(got, exp, "pair rounds at the gate")


@gpu
def test_one_chunk_pair_below_the_gate():
    """The same rows cut to n_it = 1 022: no pair item, the same truth."""
    nb = gate_blocks(cu_count())
    M, N = 32 * (nb - 1) + 1, N_BELOW
    bed, pos, rsq, exp = band(N, M)
    (got, t), _ = run_on_off(bed, M, N, pos, rsq)
    assert t["band_kernel"] != "f4_colpair" and pair_lists(t) == (0, 0, 0), t
    check_multiplicity(got, exp, "n_it 1022")


@gpu
def test_one_block_below_two_rounds():
    """One block fewer: fewer than two rounds of pairs (and of block pairs), no pair item."""
    n_cu = cu_count()
    nb = gate_blocks(n_cu) - 1
    M, N = 32 * nb, N_GATE
    assert sum(n // 2 for n in range(1, nb + 1)) < 8 * n_cu or nb * (nb + 1) // 2 < 16 * n_cu
    bed, pos, rsq, _ = band(N, M)
    (got, t), _ = run_on_off(bed, M, N, pos, rsq)
    assert t["band_kernel"] != "f4_colpair" and pair_lists(t) == (0, 0, 0), t


# ---------------------------------------------------------------------------------------------------------------
# the patterns all-missing rows cannot reach, at 1 024 chunks
# ---------------------------------------------------------------------------------------------------------------

N_LONG = (1 << 17) - 1


def block_end_targets(M):
    """Both ends of every 32-SNP block, and SNPs inside until there are at least 32."""
    t = {x for b in range((M + 31) // 32) for x in (32 * b, min(M, 32 * b + 32) - 1)}
    t |= set(np.random.default_rng(M).choice(M, 32, replace=False).tolist())
    return np.array(sorted(t), np.int64)


def check_targets(got, rows, bed, N, args, label):
    wind, maf, std_thr, rsq, pos = args
    t = block_end_targets(len(pos))
    O.code_counts(bed, len(pos), N, threads=THREADS)  # (sets the oracle's OpenMP team size)
    assert len(t) >= 32
    pairs = O.pair_r2_f64(rows, N, wind, maf, std_thr, pos, t)
    r2d = np.concatenate([p[3] for p in pairs if p is not None])
    assert np.abs(r2d - rsq).min() > 1e-9, label  # (WSDE compared exactly)
    exp = O.run_f64_targets(rows, N, wind, maf, std_thr, rsq, pos, t)
    sub = {k: v[t] for k, v in got.items()}
    assert_ld_close(sub, exp, tol=EXACT, label=label)
    np.testing.assert_array_equal(sub["l2d_wse"], exp["l2d_wse"], err_msg=label)


@gpu
def test_long_rows_row_and_column_missing_patterns():
    """The four (row, columns) missingness instantiations of the pair loop at 1 024 chunks."""
    N = N_LONG
    rows, bed, M, args, round_items, options = missing_patterns_case(N)
    got, _ = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items, options=options)
    check_targets(got, rows, bed, N, args, "long rows, missing patterns")


@gpu
@pytest.mark.parametrize("t2,shift", [(3, 2), (1, 1)], ids=["quad", "2x2"])
def test_long_rows_routing_drops_one_block_of_a_pair(t2, shift):
    """The lose-one-block body of the pair kernel at 1 024 chunks, beside both super-item kernels."""
    N = N_LONG
    rows, bed, M, args, round_items, options, _ = routing_case(N, t2, shift)
    got, _ = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=round_items, options=options)
    check_targets(got, rows, bed, N, args, f"long rows, routing t2 {t2}")


@gpu
@pytest.mark.parametrize("defer", [1, 0], ids=["deferred", "kc_launch"])
def test_long_rows_one_replayed_block_in_a_pair(defer):
    """The rep_gram partial stores of a pair item (and the KC instantiation) at 1 024 chunks."""
    N = N_LONG
    bed, M, args, round_items = one_replayed_case(N)
    got, _ = ab(bed, M, N, args, flags=F4, round_items=round_items, options={"defer_rep": defer})
    if defer:
        assert_ld_close(got, O.run_c(bed, M, N, *args), label="long rows, one replayed block vs oracle")


@gpu
def test_missing_patterns_below_the_chunk_gate_take_no_pair_items():
    """N = 32 773 (n_it = 258), no round option: below the n_it gate the run takes no pair item and equals the
    f4_nc2_dom 0 run."""
    N = 32_773
    rows, bed, M, args, _, options = missing_patterns_case(N)
    got, t = ab(bed, M, N, args, flags=F4 | flag("FLAG_EXACT_RARE"), round_items=0, options=options,
                want=("f4", "f4_ksplit"))
    assert pair_lists(t) == (0, 0, 0), t
