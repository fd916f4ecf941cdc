"""Keep-list loads on long rows: sparse, dense and clustered lists through `subset_samples_kernel`.

The contract is tests/test_gpu_keep.py's: a keep-load followed by a run equals, bit for bit in all seven result arrays,
a plain load of the numpy-subsetted bytes (`subset_rows`) run with NLDSC_FLAG_STRICT_PLINK_ORDER, and that plain load
lies within `tol_for(mode)` of the C oracle in strict order on the same bytes.  That module's rows are 250 / 251 bytes,
shorter than one SUB_PIECE: every workgroup there gathers its samples from a single piece.  Here the rows are 10 to
21 KB and the lists are built so that the kernel's piece walk takes every branch: many pieces, skipped gaps, one piece
per code, a piece that begins exactly where the one before ended, workgroup and word boundaries in n_keep, a span
that ends on the file row's last byte.  `piece_walk` restates the walk; every case first asserts on the CPU that it
reaches the class it was built for.

Rows: M = 70 (two full 32-row groups and one of 6), independent genotypes with a per-SNP A2 frequency uniform in
[0.25, 0.75] (both stored orientations) and 1 % missing calls.  Two different samples then differ in a given row with
probability >= 0.37, so one mis-gathered sample escapes all 70 rows with probability < 1e-14, and any change of a
count moves MAF bitwise.  One window over all SNPs: every row meets every other row."""
import functools

import numpy as np
import pytest

from conftest import assert_ld_close, tol_for
from oracle import oracle as O
from test_gpu_keep import MODES, STRICT, assert_bitwise, run_modes, subset_rows

pytestmark = pytest.mark.gpu

SUB_WORDS = 64   # ld_kernels.hip: output words of 16 codes per workgroup
SUB_PIECE = 512  # ld_kernels.hip: source bytes per row and piece
WG_CODES = SUB_WORDS * 16  # 1 024 kept samples per workgroup

M = 70
POS = 0.01 * np.arange(M)
META = dict(ld_wind=1.0, maf=0.01, std_thr=1e-5, rsq_thr=1.0 / M)  # (ld_wind above the span of 0.69)
DEFAULT = {"default": 0}  # flags 0: the engine's default band mode


def piece_walk(idx):
    """Per workgroup of WG_CODES kept samples: (pieces, skipped gaps) of subset_samples_kernel's walk over the source
    bytes idx >> 2: a piece covers [pb, pb + SUB_PIECE), the next starts at the first byte >= pb + SUB_PIECE that holds
    a code of the workgroup (a gap where that byte lies further on)."""
    out = []
    for first in range(0, len(idx), WG_CODES):
        b = np.asarray(idx[first:first + WG_CODES], np.int64) >> 2
        pb, pieces, gaps = int(b[0]), 1, 0
        while True:
            k = np.searchsorted(b, pb + SUB_PIECE)
            if k == len(b):
                break
            gaps += int(b[k] > pb + SUB_PIECE)
            pb, pieces = int(b[k]), pieces + 1
        out.append((pieces, gaps))
    return out


def n_wr(n_keep: int) -> int:
    """Workgroups per 32 rows (launch_subset_slice)."""
    nb_dst = n_keep // 4 + (n_keep % 4 > 0)
    n_words = (nb_dst + 3) // 4
    return (n_words + SUB_WORDS - 1) // SUB_WORDS


def row_bytes(n: int) -> int:
    return n // 4 + (n % 4 > 0)


@pytest.fixture(scope="module")
def engine():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    from nldsc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def file_rows(n_file: int) -> np.ndarray:
    """The .bed rows [M][ceil(n_file / 4)] of the module's genotypes at n_file individuals (padding pairs 00)."""
    from nldsc_amd import synth
    rng = np.random.default_rng(9000 + n_file)
    p = rng.uniform(0.25, 0.75, M)[:, None]
    g = ((rng.random((M, n_file)) < p).astype(np.int8) + (rng.random((M, n_file)) < p).astype(np.int8))
    g[rng.random((M, n_file)) < 0.01] = -1
    rows = synth.pack_bed_rows(g)
    rows.setflags(write=False)
    return rows


def check_keep_load(engine, n_file: int, idx, modes=DEFAULT, label=""):
    """The contract, with the host loader and with the device loader on a tensor whose rows start at +3."""
    import torch
    from nldsc_amd import synth
    idx = np.ascontiguousarray(idx, np.int32)
    assert idx[0] >= 0 and idx[-1] < n_file and (np.diff(idx) > 0).all()
    rows = file_rows(n_file)
    sub = synth.bed_bytes(subset_rows(rows, n_file, idx))
    bed = synth.bed_bytes(rows)

    def run(extra=0):
        if modes is MODES:
            return run_modes(engine, META, POS, extra)
        return {"default": engine.run(META["ld_wind"], META["maf"], META["std_thr"], META["rsq_thr"], POS,
                                      flags=extra)}

    engine.set_keep(None)
    engine.load_bed_bytes(sub, M, len(idx))
    assert engine.kept() == 0 and engine.n_org == len(idx)
    exp = run(STRICT)
    orc = O.run_c(sub, M, len(idx), META["ld_wind"], META["maf"], META["std_thr"], META["rsq_thr"], POS,
                  flags=O.STRICT_ORDER)
    assert np.isfinite(orc["l2"]).all() and (orc["l2_ws"] == M - 1).all()  # every row meets every other
    for m in modes:
        assert_ld_close(exp[m], orc, tol=tol_for(m), label=f"{label} {m} subset bytes vs oracle")
    dev = torch.frombuffer(bytearray(bed), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    try:
        engine.set_keep(idx, n_file)
        for loader in ("host", "device"):
            if loader == "host":
                engine.load_bed_bytes(bed, M, n_file)
            else:
                engine.load_bed_device(dev.data_ptr(), dev.numel(), M, n_file)
            assert engine.kept() == len(idx) and engine.n_org == len(idx)
            got = run()
            for m in modes:
                assert_bitwise(got[m], exp[m], f"{label} {loader} {m}")
    finally:
        engine.set_keep(None)


# ---- lists ----------------------------------------------------------------------------------------------------------
def _everyone():
    n = 40_003
    idx = np.arange(n)
    walk = piece_walk(idx)
    assert n_wr(len(idx)) == 40 == len(walk) and all(p == 1 and g == 0 for p, g in walk)
    assert row_bytes(n) == 10_001 and idx[WG_CODES] >> 2 == 256  # the second workgroup's piece starts mid-row
    return n, idx


def _every_3rd():
    n = 40_003
    idx = np.arange(1, n, 3)
    walk = piece_walk(idx)
    assert len(idx) == 13_334 and n_wr(len(idx)) == 14 == len(walk)
    assert max(p for p, _ in walk) == 2 and any(p == 2 for p, _ in walk)
    return n, idx


def _every_8th():
    n = 40_003
    idx = np.arange(5, n, 8)
    walk = piece_walk(idx)
    assert len(idx) == 5_000 and n_wr(len(idx)) == 5 == len(walk) and all(p == 4 for p, _ in walk)
    return n, idx


def _every_37th():
    n = 40_003
    idx = np.arange(2, n, 37)
    walk = piece_walk(idx)
    assert len(idx) == 1_082 and n_wr(len(idx)) == 2 == len(walk)
    assert sum(g for _, g in walk) >= 10 and walk[0][0] >= 10
    return n, idx


def _every_2049th():
    n = 75_813
    idx = np.arange(0, n, 2_049)  # 2 049 % 4 = 1: the pair shift cycles
    walk = piece_walk(idx)
    assert n_wr(len(idx)) == 1 and walk[0][0] == len(idx) == 37 and walk[0][1] >= 1  # one piece per code
    assert set(idx[:4] & 3) == {0, 1, 2, 3}
    return n, idx


def _random_half():
    n = 66_001
    idx = np.sort(np.random.default_rng(101).choice(n, 33_000, replace=False))
    walk = piece_walk(idx)
    assert n_wr(len(idx)) == 33 == len(walk) and max(p for p, _ in walk) >= 2
    return n, idx


def _random_20th():
    n = 66_001
    idx = np.sort(np.random.default_rng(102).choice(n, 3_300, replace=False))
    walk = piece_walk(idx)
    assert n_wr(len(idx)) == 4 == len(walk) and max(p for p, _ in walk) >= 3 and sum(g for _, g in walk) >= 1
    return n, idx


def _clustered():
    n = 66_002
    rng = np.random.default_rng(103)
    runs, s = [], 3
    for _ in range(7):  # runs of 1 500 samples, 5 000 to 9 000 dropped samples between them
        runs.append(np.arange(s, s + 1_500))
        s += 1_500 + int(rng.integers(5_000, 9_001))
    idx = np.concatenate(runs)
    walk = piece_walk(idx)
    assert len(idx) == 10_500 and idx[-1] < n and n_wr(len(idx)) == 11 == len(walk)
    inside = [np.diff(idx[a:a + WG_CODES]).max() >= 5_000 for a in range(0, len(idx), WG_CODES)]
    assert any(inside) and not all(inside)  # some workgroup's words straddle a gap between runs
    assert any(g > 0 for _, g in walk)
    return n, idx


def _piece_ties():
    n = 82_228
    t = np.arange(40)
    byte = np.sort(np.concatenate([77 + SUB_PIECE * t, 77 + SUB_PIECE * t + SUB_PIECE - 1]))
    idx = 4 * byte + np.arange(len(byte)) % 4
    walk = piece_walk(idx)
    assert len(idx) == 80 and n_wr(80) == 1 and walk == [(40, 0)]  # every piece begins where the one before ended
    assert idx[-1] == n - 1 and byte[-1] == row_bytes(n) - 1  # (and the last code sits on the row's last byte)
    return n, idx


LISTS = {"everyone": (_everyone, MODES), "every_3rd_from_1": (_every_3rd, DEFAULT),
         "every_8th_from_5": (_every_8th, DEFAULT), "every_37th_from_2": (_every_37th, DEFAULT),
         "every_2049th": (_every_2049th, DEFAULT), "random_half": (_random_half, DEFAULT),
         "random_20th": (_random_20th, MODES), "clustered": (_clustered, DEFAULT), "piece_ties": (_piece_ties, MODES)}


@pytest.mark.parametrize("name", list(LISTS))
def test_lists(engine, name):
    build, modes = LISTS[name]
    n_file, idx = build()
    check_keep_load(engine, n_file, idx, modes, name)


# ---- n_keep on either side of a workgroup or word boundary ---------------------------------------------------------
@pytest.mark.parametrize("n_keep,wgs", [(1_024, 1), (1_025, 2), (2_047, 2), (2_048, 2), (2_049, 3)])
def test_boundary_counts(engine, n_keep, wgs):
    """1 025: the second workgroup owns one code and stores a single byte; 2 047: the last byte three quarters full;
    2 049: 513 compact bytes, 129 words, a third workgroup."""
    n_file = 40_002
    idx = np.sort(np.random.default_rng(200 + n_keep).choice(n_file, n_keep, replace=False))
    assert n_wr(n_keep) == wgs == len(piece_walk(idx))
    if n_keep == 2_049:
        assert row_bytes(n_keep) == 513 and (513 + 3) // 4 == 129
    check_keep_load(engine, n_file, idx, label=f"n_keep {n_keep}")


# ---- a span that ends on the file row's last byte, in a later piece ----------------------------------------------------
@pytest.mark.parametrize("n_file,mod16", [(40_000, 0), (40_001, 1), (40_002, 1), (40_003, 1), (40_060, 15)])
def test_row_ends(engine, n_file, mod16):
    """[0 .. 2 044] + [n_file - 1]: the last workgroup skips from byte 511 to the row's last byte, a unit read byte by
    byte unless the row is whole 16-byte units; the last sample sits in each of the four pairs of its byte."""
    idx = np.concatenate([np.arange(2_045), [n_file - 1]])
    walk = piece_walk(idx)
    assert row_bytes(n_file) % 16 == mod16 and idx[-1] >> 2 == row_bytes(n_file) - 1
    assert n_wr(len(idx)) == 2 and walk == [(1, 0), (2, 1)] and idx[-2] >> 2 == 511
    assert (n_file - 1) % 4 == {40_000: 3, 40_001: 0, 40_002: 1, 40_003: 2, 40_060: 3}[n_file]
    check_keep_load(engine, n_file, idx, label=f"row ends {n_file}")


# ---- removing a few people -------------------------------------------------------------------------------------------
def _removed(which, n_file):
    if which == "random_1pct":
        return np.sort(np.random.default_rng(300).choice(n_file, n_file // 100, replace=False))
    return np.array([{"first": 0, "last": n_file - 1, "middle": 20_001}[which]])


@pytest.mark.parametrize("which", ["first", "last", "middle", "random_1pct"])
def test_remove_a_few(engine, which):
    """From the removed sample on, every workgroup's quarter piece is shifted by one sample."""
    n_file = 40_003
    idx = np.setdiff1d(np.arange(n_file), _removed(which, n_file))
    walk = piece_walk(idx)
    assert n_wr(len(idx)) == len(walk) >= 39 and all(p <= 2 and g == 0 for p, g in walk)
    check_keep_load(engine, n_file, idx, label=f"remove {which}")
