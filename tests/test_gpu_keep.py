"""LD scores on a subset of the individuals (nldsc_engine_set_keep, --keep / --remove).

The contract: a keep-load followed by a run equals, bit for bit in all seven result arrays, a plain load of the
physically subsetted .bed (what `plink --keep` writes) run with NLDSC_FLAG_STRICT_PLINK_ORDER.  The expected bytes
come from numpy here (unpack in PLINK order, select columns, repack); the plain load is the engine's own, compared
with the oracle in strict mode at the usual tolerances."""
import ctypes
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, assert_ld_close, load_set, rare_variant_set, tol_for
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")
MODES = {"f32": 8, "i8": 4, "f4": 16}  # _lib.FLAG_FP32, _lib.FLAG_EXACT_I8, _lib.FLAG_EXACT_F4
STRICT = 1  # _lib.FLAG_STRICT_PLINK_ORDER


@pytest.fixture(scope="module")
def engine():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    from nldsc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_GENO_OF_CODE = np.array([0, -1, 1, 2], np.int8)  # bit pair -> A2 count (01: missing)


def subset_rows(rows: np.ndarray, n_org: int, idx) -> np.ndarray:
    """The .bed rows `plink --keep` writes: samples `idx` (PLINK order) of rows [M][ceil(n_org / 4)], repacked."""
    from nldsc_amd import synth
    out = []
    for a in range(0, len(rows), 128):  # (in row chunks: the unpacked codes are 4 bytes per .bed byte)
        codes = O.unpack_codes(rows[a:a + 128], n_org, strict=True)[:, idx]
        out.append(synth.pack_bed_rows(_GENO_OF_CODE[codes]))
    return np.concatenate(out)


def assert_bitwise(got: dict, exp: dict, label=""):
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k], equal_nan=got[k].dtype.kind == "f"), \
            f"{label}: {k} differs at {np.flatnonzero(~((got[k] == exp[k]) | ((got[k] != got[k]) & (exp[k] != exp[k]))))[:10]}"


def keep_lists(N: int) -> dict:
    rng = np.random.default_rng(4000 + N)
    out = {"everyone": np.arange(N), "every_second": np.arange(0, N, 2)}
    for r in range(4):  # n_keep % 4 = r
        out[f"random_rem{r}"] = np.sort(rng.choice(N, 4 * int(rng.integers(60, 200)) + r, replace=False))
    out["contiguous_from_5"] = np.arange(5, 5 + 4 * 77 + 1)  # an unaligned start, n_keep % 4 = 1
    out["ends_and_sparse"] = np.concatenate([[0], np.sort(rng.choice(np.arange(1, N - 1), 97, replace=False)), [N - 1]])
    out["one"] = np.array([int(rng.integers(0, N))])
    return {k: v.astype(np.int32) for k, v in out.items()}


LIST_NAMES = sorted(keep_lists(1000))
_sets: dict = {}


def golden(name):
    """(rows, positions, meta) of a committed fixture, read once."""
    if name not in _sets:
        bed, pos, meta, _, _ = load_set(name)
        _sets[name] = (np.frombuffer(bed, np.uint8, offset=3).reshape(meta["n_snp"], -1), pos, meta, bed)
    return _sets[name]


def run_modes(engine, meta, pos, extra_flags=0):
    return {m: engine.run(meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"], pos, flags=f | extra_flags)
            for m, f in MODES.items()}


@pytest.mark.parametrize("which", LIST_NAMES)
@pytest.mark.parametrize("name", ["n1000", "n1001", "n1002", "n1003"])
def test_keep_load_equals_plain_load_of_the_subset(engine, name, which):
    """Golden fixtures (source rows of 250 / 251 bytes: odd-aligned), every keep list, host and device loaders, the
    three band modes: bitwise the plain load of the subset bytes run strict; that one within TOL of the oracle (which
    refuses cohorts below three: the list of one is compared bitwise only)."""
    import torch
    from nldsc_amd import synth
    rows, pos, meta, bed = golden(name)
    M, N = meta["n_snp"], meta["n_org"]
    idx = keep_lists(N)[which]
    sub = synth.bed_bytes(subset_rows(rows, N, idx))
    engine.set_keep(None)
    engine.load_bed_bytes(sub, M, len(idx))
    assert engine.kept() == 0 and engine.n_org == len(idx)
    exp = run_modes(engine, meta, pos, STRICT)
    orc = None
    if len(idx) > 2:
        orc = O.run_c(sub, M, len(idx), meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"], pos,
                      flags=O.STRICT_ORDER)
        for m in MODES:
            assert_ld_close(exp[m], orc, tol=tol_for(m), label=f"{name} {which} {m} subset file vs oracle")
    dev = torch.frombuffer(bytearray(bed), dtype=torch.uint8).cuda()  # (the rows start at +3: no alignment)
    torch.cuda.synchronize()
    try:
        engine.set_keep(idx, N)
        for loader in ("host", "device"):
            if loader == "host":
                engine.load_bed_bytes(bed, M, N)
            else:
                engine.load_bed_device(dev.data_ptr(), dev.numel(), M, N)
            assert engine.kept() == len(idx) and engine.n_org == len(idx)
            got = run_modes(engine, meta, pos)
            for m in MODES:
                assert_bitwise(got[m], exp[m], f"{name} {which} {loader} {m}")
                if orc is not None:
                    assert_ld_close(got[m], orc, tol=tol_for(m), label=f"{name} {which} {loader} {m} vs oracle")
    finally:
        engine.set_keep(None)


def test_keep_everyone_is_the_strict_run(engine):
    rows, pos, meta, bed = golden("n1001")
    M, N = meta["n_snp"], meta["n_org"]
    engine.set_keep(None)
    engine.load_bed_bytes(bed, M, N)
    exp = run_modes(engine, meta, pos, STRICT)
    compat = run_modes(engine, meta, pos)
    assert not np.array_equal(compat["f4"]["l2"], exp["f4"]["l2"], equal_nan=True)  # N % 4 = 1: the order matters
    try:
        engine.set_keep(np.arange(N), N)
        engine.load_bed_bytes(bed, M, N)
        assert engine.kept() == N
        got, got_strict = run_modes(engine, meta, pos), run_modes(engine, meta, pos, STRICT)
        for m in MODES:
            assert_bitwise(got[m], exp[m], f"keep everyone {m}")
            assert_bitwise(got_strict[m], exp[m], f"keep everyone, strict flag {m}")
        engine.set_keep(None)
        assert engine.kept() == N  # (the list affects the next loads only)
        engine.load_bed_bytes(bed, M, N)
        assert engine.kept() == 0 and engine.n_org == N
        again = run_modes(engine, meta, pos)
        for m in MODES:
            assert_bitwise(again[m], compat[m], f"plain reload {m}")
    finally:
        engine.set_keep(None)


def test_missing_rich_rows_keep_half(engine):
    """Rare variants (replayed residuals), A1-minor rows (orientation) and 1 % missing calls on compacted rows."""
    from nldsc_amd import synth
    N = 1003
    rows, pos = rare_variant_set(N)
    M = len(rows)
    idx = np.sort(np.random.default_rng(11).choice(N, N // 2, replace=False)).astype(np.int32)
    sub = synth.bed_bytes(subset_rows(rows, N, idx))
    meta = dict(ld_wind=1.0, maf=1e-5, std_thr=1e-5, rsq_thr=1.0 / M)
    engine.set_keep(None)
    engine.load_bed_bytes(sub, M, len(idx))
    exp = run_modes(engine, meta, pos, STRICT)
    orc = O.run_c(sub, M, len(idx), 1.0, 1e-5, 1e-5, 1.0 / M, pos, flags=O.STRICT_ORDER)
    try:
        engine.set_keep(idx, N)
        engine.load_bed_bytes(synth.bed_bytes(rows), M, N)
        got = run_modes(engine, meta, pos)
    finally:
        engine.set_keep(None)
    for m in MODES:
        assert_bitwise(got[m], exp[m], f"rare {m}")
        assert_ld_close(got[m], orc, tol=tol_for(m), label=f"rare {m} vs oracle")


SLICE_BYTES = 64 << 20  # ld_engine.cpp: the host and device loaders' staging slices


def loader_slices(n_rows: int, row_bytes: int) -> list:
    """Rows per staging slice of nldsc_engine_load_bed_host (row_bytes: the file's rows) and of
    nldsc_engine_load_bed_device with a list (row_bytes: the compact rows): ~64 MiB of whole 32-SNP blocks."""
    rows_per = max(32, SLICE_BYTES // row_bytes // 32 * 32)
    return [min(rows_per, n_rows - r0) for r0 in range(0, n_rows, rows_per)]


@pytest.fixture(scope="module")
def long_rows(tmp_path_factory):
    """N = 315 599 (rows of 78 900 bytes), M = 900, a random half of the individuals and the rows `plink --keep`
    writes for them (~4 s of numpy), both as .bed files too."""
    N, M = 315_599, 900
    nb = (N + 3) // 4
    rng = np.random.default_rng(77)
    # every pair one of hom A1 / het / hom A2 (from uniform bytes through a 256-entry table), then ~0.4 % of the bytes
    # with a missing call, and 00 in the last byte's padding pair
    pair = np.array([0, 2, 3, 0], np.uint8)
    b = np.arange(256)
    lut = (pair[b & 3] | (pair[(b >> 2) & 3] << 2) | (pair[(b >> 4) & 3] << 4) | (pair[(b >> 6) & 3] << 6)).astype(np.uint8)
    rows = lut[rng.integers(0, 256, (M, nb), dtype=np.uint8)]
    hit = rng.integers(0, M * nb, M * nb // 256)
    rows.reshape(-1)[hit] = (rows.reshape(-1)[hit] & 0xFC) | 1
    rows[:, -1] &= 0x3F
    idx = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    sub = subset_rows(rows, N, idx)
    d = tmp_path_factory.mktemp("long_rows")
    src, dst = d / "full.bed", d / "sub.bed"
    with open(src, "wb") as fh:
        fh.write(b"\x6c\x1b\x01")
        fh.write(rows.tobytes())
    with open(dst, "wb") as fh:
        fh.write(b"\x6c\x1b\x01")
        fh.write(sub.tobytes())
    pos = np.cumsum(rng.exponential(0.02, M))
    rows.setflags(write=False)
    return dict(N=N, M=M, rows=rows, idx=idx, src=src, dst=dst, pos=pos, args=(1.0, 0.01, 1e-5, 1.0 / M))


def test_multi_slice_file_reader(engine, long_rows):
    """The expected file takes ~4 s of numpy per 1 000 rows: three reader slices of 416, 416 and 68 rows, each on its
    own thread, slot and stream; the whole file and the row range [200, 700) (two slices)."""
    N, M, idx, src, dst, pos, args = (long_rows[k] for k in ("N", "M", "idx", "src", "dst", "pos", "args"))
    engine.set_keep(None)
    engine.load_bed_file(str(dst), M, len(idx))
    exp = engine.run(*args, pos, flags=STRICT)
    engine.load_bed_file_range(str(dst), M, len(idx), 200, 700)
    exp_range = engine.run(*args, pos[200:700], flags=STRICT)
    try:
        engine.set_keep(idx, N)
        engine.load_bed_file(str(src), M, N)
        assert engine.kept() == len(idx) and engine.n_snp == M
        got = engine.run(*args, pos)
        engine.load_bed_file_range(str(src), M, N, 200, 700)
        assert engine.kept() == len(idx) and engine.n_snp == 500
        got_range = engine.run(*args, pos[200:700])
    finally:
        engine.set_keep(None)
    assert np.isfinite(exp["l2"]).sum() > M // 2
    assert_bitwise(got, exp, "file")
    assert_bitwise(got_range, exp_range, "file range")


def test_multi_slice_host_loader(engine, long_rows):
    """The host loader with the half list on the same rows: the 71 MB source goes up in two slices of 832 and 68 rows,
    the second over both staging regions (source rows and compact rows) of the first.  Bitwise the file loader's
    result, and the plain load's of the subset file."""
    N, M, idx, src, dst, pos, args = (long_rows[k] for k in ("N", "M", "idx", "src", "dst", "pos", "args"))
    assert loader_slices(M, (N + 3) // 4) == [832, 68]
    engine.set_keep(None)
    engine.load_bed_file(str(dst), M, len(idx))
    exp = engine.run(*args, pos, flags=STRICT)
    bed = np.fromfile(src, np.uint8)
    try:
        engine.set_keep(idx, N)
        engine.load_bed_file(str(src), M, N)
        by_file = engine.run(*args, pos)
        engine.load_bed_bytes(bed, M, N)
        assert engine.kept() == len(idx) and engine.n_snp == M
        got = engine.run(*args, pos)
    finally:
        engine.set_keep(None)
    assert_bitwise(got, by_file, "host loader vs file loader")
    assert_bitwise(got, exp, "host loader vs the subset file")


def test_multi_slice_device_loader_three_removed(engine, long_rows):
    """The device loader slices by compact rows: with the first, a middle and the last individual removed they are
    78 899 bytes, 832 + 68 rows again.  Bitwise the plain load of the subset bytes (a second ~4 s of numpy)."""
    import torch
    N, M, rows, src, pos, args = (long_rows[k] for k in ("N", "M", "rows", "src", "pos", "args"))
    idx = np.setdiff1d(np.arange(N), [0, N // 2, N - 1]).astype(np.int32)
    nb_img = (len(idx) + 3) // 4
    assert nb_img == 78_899 and len(loader_slices(M, nb_img)) >= 2 and loader_slices(M, nb_img)[0] % 32 == 0
    sub = subset_rows(rows, N, idx)
    engine.set_keep(None)
    engine.load_bed_bytes(np.concatenate([np.frombuffer(b"\x6c\x1b\x01", np.uint8), sub.reshape(-1)]), M, len(idx))
    exp = engine.run(*args, pos, flags=STRICT)
    dev = torch.from_numpy(np.fromfile(src, np.uint8)).cuda()  # (the rows start at +3: no alignment)
    torch.cuda.synchronize()
    try:
        engine.set_keep(idx, N)
        engine.load_bed_device(dev.data_ptr(), dev.numel(), M, N)
        assert engine.kept() == len(idx) and engine.n_snp == M
        got = engine.run(*args, pos)
    finally:
        engine.set_keep(None)
    assert np.isfinite(exp["l2"]).sum() > M // 2
    assert_bitwise(got, exp, "device loader, three removed")


def test_index_validation_and_load_errors(engine, tmp_path):
    from nldsc_amd import _lib
    rows, pos, meta, bed = golden("n1001")
    M, N = meta["n_snp"], meta["n_org"]
    L, h = engine._L, engine._h

    def set_keep_rc(values, n_keep=None, n_file=N):
        a = np.asarray(values, np.int32)
        err = _lib.errbuf()
        return L.nldsc_engine_set_keep(h, a.ctypes.data, len(a) if n_keep is None else n_keep, n_file, err, len(err))

    engine.set_keep(None)
    for bad in ([5, 4, 3], [1, 2, 2, 3], [-1, 0, 1], [0, 1, N], [0, N + 5]):
        assert set_keep_rc(bad) == _lib.E_ARG, bad
    assert set_keep_rc([0, 1, 2], n_keep=0) == _lib.E_ARG  # n_keep = 0 with a list
    assert set_keep_rc(list(range(9)), n_file=8) == _lib.E_ARG  # more kept than the file holds
    # a rejected list leaves none set: the next load is a plain one
    engine.load_bed_bytes(bed, M, N)
    assert engine.kept() == 0
    try:
        engine.set_keep([0, 2, 4, 6, 100], N)
        with pytest.raises(_lib.NLDSCError) as ex:
            engine.load_bed_bytes(bed, M, N - 1)  # n_org is not the list's file count
        assert ex.value.code == _lib.E_ARG
        with pytest.raises(_lib.NLDSCError) as ex:
            engine.load_bed_file(os.path.join(GOLDEN, "n1001.bed"), M, 5)
        assert ex.value.code == _lib.E_ARG
        # a .bed too short for the file's individuals: the size check runs against the file's n_org
        short = bytes(bed[:3 + (M - 1) * rows.shape[1]])
        with pytest.raises(_lib.NLDSCError, match=f"{M} SNPs x {N} individuals") as ex:
            engine.load_bed_bytes(short, M, N)
        assert ex.value.code == _lib.E_SIZE
        (tmp_path / "short.bed").write_bytes(short)
        with pytest.raises(_lib.NLDSCError, match=f"{M} SNPs x {N} individuals") as ex:
            engine.load_bed_file(str(tmp_path / "short.bed"), M, N)
        assert ex.value.code == _lib.E_SIZE
        # a run with the file's n_org does not match the image of 5
        engine.load_bed_bytes(bed, M, N)
        p, _pos = _lib.make_params(M, N, 1.0, 0.01, 1e-5, 1e-3, pos)
        arrs, res = _lib.alloc_result(M)
        err = _lib.errbuf()
        assert L.nldsc_engine_run(h, ctypes.byref(p), 0, M, ctypes.byref(res), err, len(err)) == _lib.E_ARG
    finally:
        engine.set_keep(None)


@pytest.fixture(scope="module")
def keep_case(engine, tmp_path_factory):
    """n1001 with a keep file, a remove file and the physically subsetted file set; the engine's result (default mode)."""
    from nldsc_amd import synth
    d = tmp_path_factory.mktemp("keep")
    rows, pos, meta, bed = golden("n1001")
    M, N = meta["n_snp"], meta["n_org"]
    rng = np.random.default_rng(5)
    listed = np.sort(rng.choice(N, 600, replace=False))
    removed = np.sort(rng.choice(listed, 90, replace=False))
    idx = np.setdiff1d(listed, removed).astype(np.int32)
    fam = open(os.path.join(GOLDEN, "n1001.fam")).read().splitlines()
    ids = [ln.split()[:2] for ln in fam]
    (d / "keep.txt").write_text("".join(f"{ids[s][0]} {ids[s][1]}\n" for s in rng.permutation(listed)) + "NO BODY\n")
    (d / "remove.txt").write_text("".join(f"{ids[s][0]}\t{ids[s][1]}\tx\n" for s in removed))
    (d / "sub.bed").write_bytes(synth.bed_bytes(subset_rows(rows, N, idx)))
    (d / "sub.fam").write_text("".join(fam[s] + "\n" for s in idx))
    shutil.copy(os.path.join(GOLDEN, "n1001.bim"), d / "sub.bim")
    engine.set_keep(None)
    engine.load_bed_bytes((d / "sub.bed").read_bytes(), M, len(idx))
    exp = engine.run(meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"], pos, flags=STRICT)
    return d, idx, exp


def test_one_shot_calls(keep_case):
    from nldsc_amd import engine as E
    from nldsc_amd.ldscore import _ldscore as lds
    d, idx, exp = keep_case
    _, pos, meta, _ = golden("n1001")
    path = os.path.join(GOLDEN, "n1001.bed")
    got = E.calculate(path, meta["n_snp"], meta["n_org"], meta["ld_wind"], meta["maf"], meta["std_thr"],
                      meta["rsq_thr"], pos, keep=idx)
    assert_bitwise(got, exp, "engine.calculate(keep=)")
    p = lds.LDScoreParams(path, n_snp=meta["n_snp"], n_org=meta["n_org"], ld_wind=meta["ld_wind"], maf=meta["maf"],
                          std_thr=meta["std_thr"], rsq_thr=meta["rsq_thr"], positions=pos.tolist())
    p.keep = idx.tolist()
    r = lds.calculate(p)
    assert_bitwise({k: np.asarray(getattr(r, k), dtype=exp[k].dtype) for k in KEYS}, exp, "pybind calculate")
    p.keep = idx[::-1].tolist()
    with pytest.raises(RuntimeError, match="keep list"):
        lds.calculate(p)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ld(args, *, ranks=1, timeout=300):
    """The CLI, as tests/test_gpu_torchrun.py starts it (gloo: both ranks on GPU 0)."""
    env = dict(os.environ, NLDSC_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    if ranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "-m", "nldsc_amd", "ld"] + args
    else:
        cmd = [sys.executable, "-m", "nldsc_amd", "ld"] + args
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0 and "crashed" not in p.stderr, p.stderr[-3000:]
    return p


@pytest.fixture(scope="module")
def cli_keep_run(keep_case):
    d = keep_case[0]
    common = ["--ld-wind-cm", "1", "-maf", "0.01", "--extra", "--write-m", "--quiet"]
    p = _ld(["--bfile", os.path.join(GOLDEN, "n1001"), "--keep", str(d / "keep.txt"), "--remove",
             str(d / "remove.txt"), "--out", str(d / "keep.L2")] + common)
    return d, common, p


def test_cli_keep_remove_equals_the_subset_fileset(cli_keep_run, keep_case):
    d, common, p = cli_keep_run
    assert f"N = {len(keep_case[1])} of 1001" in p.stderr
    assert "1 of 601 IDs are not in" in p.stderr  # NO BODY
    _ld(["--bfile", str(d / "sub"), "--strict-plink-order", "--out", str(d / "sub.L2")] + common)
    assert (d / "keep.L2").read_bytes() == (d / "sub.L2").read_bytes()
    assert (d / "keep.M").read_bytes() == (d / "sub.M").read_bytes()
    assert len((d / "keep.L2").read_text().splitlines()) == 1 + 1200  # rows are SNPs


def test_cli_keep_two_ranks(cli_keep_run):
    d, common, _ = cli_keep_run
    _ld(["--bfile", os.path.join(GOLDEN, "n1001"), "--keep", str(d / "keep.txt"), "--remove", str(d / "remove.txt"),
         "--out", str(d / "two.L2")] + common, ranks=2)
    assert (d / "two.L2").read_bytes() == (d / "keep.L2").read_bytes()
    assert (d / "two.M").read_bytes() == (d / "keep.M").read_bytes()
