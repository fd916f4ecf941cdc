"""Python handle on the GPU engine (C ABI `nldsc_engine_*`, include/nldsc_ld.h).

`Engine` keeps a .bed image resident in HBM and runs the LD-score hot path over it; it is
what the benchmark, the GPU parity tests and the multi-GPU driver use.  `calculate` is the
one-shot equivalent of the reference's `_ldscore.calculate(params)`
(nldsc/ldscore/_ldscore/ldscalc.h:8-65).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

# nldsc_engine_band_kernel codes (include/nldsc_ld.h NLDSC_BAND_*)
BAND_KERNELS = {0: "f32", 1: "i8", 2: "f4", 3: "f4_seg", 4: "f4_ksplit", 5: "f4_2x2", 6: "f4_routed",
                7: "f4_quad", 8: "f4_colpair"}


def _torch_ready(*tensors):
    """Device tensors handed to the engine were written on torch's current stream (fills, copies, collectives:
    with RCCL, `req.wait()` only orders torch's stream); the engine runs on its own non-blocking HIP stream, so
    the host waits for torch's stream first."""
    import torch
    for d in {t.device for t in tensors if t is not None and t.is_cuda}:
        torch.cuda.current_stream(d).synchronize()


class Engine:
    # Engine options (C ABI nldsc_engine_set_option) applied to every new engine before `options`: test and study
    # knobs of the schedule and kernel choice (all paths give the same results: the GPU tests compare them), empty by
    # default.  See nldsc_amd/csrc/ld_engine.cpp nldsc_engine_set_option for the names.
    default_options: dict = {}

    def __init__(self, device: int = -1, lib_path: str | None = None, options: dict | None = None):
        self._L = L = _lib.lib(lib_path)
        self._h = ctypes.c_void_p()
        err = _lib.errbuf()
        _lib.check(L.nldsc_engine_create(int(device), ctypes.byref(self._h), err, len(err)), err)
        self.n_snp = 0
        self.n_org = 0
        for name, value in {**Engine.default_options, **(options or {})}.items():
            self.set_option(name, value)

    def set_option(self, name: str, value: int):
        """One engine option (nldsc_engine_set_option); "orient" applies from the next load."""
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_set_option(self._h, name.encode(), int(value), err, len(err)), err)

    def close(self):
        if self._h:
            self._L.nldsc_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- loading ------------------------------------------------------------------------
    def set_keep(self, indices, n_org_file: int = 0):
        """Keep only these individuals in the next loads (C ABI nldsc_engine_set_keep): `indices` are 0-based .fam
        line numbers, strictly ascending, of a file of n_org_file individuals; None (or empty) clears the list.  With
        a list the loaders take n_org = n_org_file and leave `self.n_org` at the kept count; runs on such an image
        use PLINK's sample order whatever their flags."""
        err = _lib.errbuf()
        if indices is None or len(indices) == 0:
            _lib.check(self._L.nldsc_engine_set_keep(self._h, None, 0, 0, err, len(err)), err)
            return
        idx = np.asarray(indices)
        if idx.ndim != 1 or idx.dtype.kind not in "iu" or (idx.size and (idx.min() < -2**31 or idx.max() >= 2**31)):
            raise ValueError("keep indices must be a 1-D sequence of 32-bit integers")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        _lib.check(self._L.nldsc_engine_set_keep(self._h, idx.ctypes.data, len(idx), int(n_org_file), err, len(err)),
                   err)

    def kept(self) -> int:
        """Kept individuals of the resident image when it was loaded with a keep list, else 0."""
        return int(self._L.nldsc_engine_kept(self._h))

    def _loaded(self, n_snp: int, n_org: int):
        k = self.kept() if hasattr(self._L, "nldsc_engine_kept") else 0
        self.n_snp, self.n_org = n_snp, (k if k > 0 else n_org)

    def load_bed_file(self, path: str, n_snp: int, n_org: int):
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_load_bed_file(self._h, path.encode(), n_snp, n_org, err, len(err)), err)
        self._loaded(n_snp, n_org)

    def load_bed_file_range(self, path: str, n_snp_file: int, n_org: int, begin: int, end: int):
        """Rows [begin, end) of a .bed file of n_snp_file SNPs (position sharding: own range + halo)."""
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_load_bed_file_range(self._h, path.encode(), n_snp_file, n_org, int(begin),
                                                               int(end), err, len(err)), err)
        self._loaded(int(end) - int(begin), n_org)

    def load_bed_bytes(self, bed, n_snp: int, n_org: int):
        """`bed`: the whole .bed content (bytes / uint8 numpy array), magic included."""
        buf = np.frombuffer(bed, dtype=np.uint8) if isinstance(bed, (bytes, bytearray)) else np.ascontiguousarray(bed, np.uint8)
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_load_bed_host(self._h, buf.ctypes.data, buf.nbytes, n_snp, n_org, err,
                                                         len(err)), err)
        self._loaded(n_snp, n_org)

    def load_bed_device(self, ptr: int, nbytes: int, n_snp: int, n_org: int):
        """Copy a .bed image that already lives in this device's memory (e.g. a torch tensor)."""
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_load_bed_device(self._h, ctypes.c_void_p(ptr), nbytes, n_snp, n_org, err,
                                                           len(err)), err)
        self._loaded(n_snp, n_org)

    # ---- compute ------------------------------------------------------------------------
    def run(self, ld_wind, maf, std_thr, rsq_thr, positions, *, own=None, flags=0, out=None, annot=None,
            covar=None):
        """LD scores for owned SNPs [own[0], own[1]) (default all).  Returns dict of numpy arrays
        (entries outside the owned range are NaN / -1, or whatever `out` held).  `annot`: an [n_snp, C] annotation
        matrix (C ABI nldsc_engine_run_annot); the dict then also holds "l2_annot" and "l2d_annot", [n_snp, C]
        float64 (taken from `out` when it has them, category-major [C, n_snp] contiguous arrays viewed transposed).
        `covar`: an [n_org, q] orthonormal basis of the centred covariates (ldscore.common.covar_basis), row i = the
        image's individual i: covariate-adjusted LD scores (C ABI nldsc_engine_run_covar), in PLINK's sample order
        (the flag is set); not together with `annot`."""
        n = self.n_snp
        own = (0, n) if own is None else own
        p, _keep = _lib.make_params(n, self.n_org, ld_wind, maf, std_thr, rsq_thr, positions, flags=flags)
        if out is None:
            arrs, res = _lib.alloc_result(n)
        else:
            arrs = out
            d, i = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
            res = _lib.Result(*(arrs[k].ctypes.data_as(d if arrs[k].dtype == np.float64 else i)
                                for k in ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")))
        err = _lib.errbuf()
        if covar is not None:
            if annot is not None:
                raise _lib.NLDSCError(_lib.E_ARG,
                                      "covariates with annotations or a pair table in one run are not supported")
            q = _lib.covar_basis_matrix(covar, self.n_org)
            p.flags |= _lib.FLAG_STRICT_PLINK_ORDER
            _lib.check(self._L.nldsc_engine_run_covar(self._h, ctypes.byref(p), q.ctypes.data, q.shape[0],
                                                      int(own[0]), int(own[1]), ctypes.byref(res), err, len(err)), err)
            return arrs
        if annot is not None:
            a = _lib.annot_matrix(annot, n)
            for k in ("l2_annot", "l2d_annot"):
                if k not in arrs:
                    arrs[k] = np.full((a.shape[0], n), np.nan).T
                if arrs[k].T.shape != a.shape or not arrs[k].T.flags.c_contiguous or arrs[k].dtype != np.float64:
                    raise ValueError(f"out['{k}'] must be the transposed view of a contiguous float64 [C, n_snp] array")
            _lib.check(self._L.nldsc_engine_run_annot(self._h, ctypes.byref(p), a.ctypes.data, a.shape[0], int(own[0]),
                                                      int(own[1]), ctypes.byref(res), arrs["l2_annot"].T.ctypes.data,
                                                      arrs["l2d_annot"].T.ctypes.data, err, len(err)), err)
            return arrs
        _lib.check(self._L.nldsc_engine_run(self._h, ctypes.byref(p), int(own[0]), int(own[1]),
                                               ctypes.byref(res), err, len(err)), err)
        return arrs

    def run_domdom(self, ld_wind, maf, std_thr, rsq_thr, positions, *, own=None, flags=0, annot=None, covar=None,
                   pairs=False):
        """`run` plus the dominance-by-dominance LD scores (C ABI nldsc_engine_run_domdom): the usual dict and
        "l2dd" (float64 [n_snp]): 1 + the sum of r2adj(R_j . R_k / N) over the pairs l2d_ws[j] counts, NaN where l2
        is NaN and where SNP j's dominance residual is constant; entries outside the owned range are NaN.  The run
        takes the closed-form vectors of rare variants (FLAG_EXACT_RARE is implied).  Annotations, covariates and a
        pair table go in runs of their own."""
        if annot is not None or covar is not None or pairs:
            raise _lib.NLDSCError(
                _lib.E_ARG, "dom-dom scores with annotations, a pair table or covariates in one run are not supported")
        n = self.n_snp
        own = (0, n) if own is None else own
        p, _keep = _lib.make_params(n, self.n_org, ld_wind, maf, std_thr, rsq_thr, positions, flags=flags)
        arrs, res = _lib.alloc_result(n)
        arrs["l2dd"] = np.full(n, np.nan)
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_run_domdom(self._h, ctypes.byref(p), int(own[0]), int(own[1]),
                                                   ctypes.byref(res), arrs["l2dd"].ctypes.data, err, len(err)), err)
        return arrs

    def covar_projections(self, n_covar: int) -> dict:
        """The projections of the last covariate run (C ABI nldsc_engine_covar_projections): "u", "w" [n_snp, q]
        (U_j = Q^T A_j in the file's allele coding, W_j = Q^T R_j), "v", "wd" [n_snp] (the shares of the additive /
        dominance-residual variance the covariates leave)."""
        n, q = self.n_snp, int(n_covar)
        u, w = np.empty((q, n)), np.empty((q, n))
        v, wd = np.empty(n), np.empty(n)
        rc = self._L.nldsc_engine_covar_projections(self._h, u.ctypes.data, w.ctypes.data, v.ctypes.data,
                                                    wd.ctypes.data)
        if rc != _lib.OK:
            raise _lib.NLDSCError(rc, "no covariate run to report projections of")
        return dict(u=u.T, w=w.T, v=v, wd=wd)

    def size_pairs(self, ld_wind, maf, std_thr, rsq_thr, positions, *, own=None, flags=0, min_r2=None):
        """The sizing call of `run_pairs` alone (C ABI nldsc_engine_run_pairs without arrays): the usual dict plus
        "row_ptr" (int64, own[1] - own[0] + 1) and "n_pairs"."""
        return self._pairs(ld_wind, maf, std_thr, rsq_thr, positions, own, flags, min_r2, emit=False)

    def run_pairs(self, ld_wind, maf, std_thr, rsq_thr, positions, *, own=None, flags=0, min_r2=None):
        """`run` plus the pairwise LD table of the owned SNPs (C ABI nldsc_engine_run_pairs: a sizing call, then the
        emitting call into arrays of that size).  The dict also holds the CSR table: "row_ptr" (int64, own[1] - own[0]
        + 1; row j - own[0] is SNP j's), "k" (int32: the neighbour, ascending within a row), "r" (float64: the
        additive correlation) and "rd" (float64: corr(A_j, R_k), NaN where the pair is not in l2d_ws[j]); with
        `min_r2` only the entries whose r2adj(r) or r2adj(rd) exceeds it."""
        return self._pairs(ld_wind, maf, std_thr, rsq_thr, positions, own, flags, min_r2, emit=True)

    def _pairs(self, ld_wind, maf, std_thr, rsq_thr, positions, own, flags, min_r2, emit, cap=None):
        n = self.n_snp
        own = (0, n) if own is None else own
        p, _keep = _lib.make_params(n, self.n_org, ld_wind, maf, std_thr, rsq_thr, positions, flags=flags)
        arrs, res = _lib.alloc_result(n)
        thr = float("nan") if min_r2 is None else float(min_r2)
        row_ptr = np.zeros(max(int(own[1]) - int(own[0]), 0) + 1, np.int64)
        n_pairs = ctypes.c_int64(0)

        def call(k, r, rd, cap_):
            err = _lib.errbuf()
            rc = self._L.nldsc_engine_run_pairs(
                self._h, ctypes.byref(p), int(own[0]), int(own[1]), ctypes.byref(res), thr, row_ptr.ctypes.data,
                None if k is None else k.ctypes.data, None if r is None else r.ctypes.data,
                None if rd is None else rd.ctypes.data, int(cap_), ctypes.byref(n_pairs), err, len(err))
            return rc, err

        if cap is None:
            rc, err = call(None, None, None, 0)
            if rc not in (_lib.OK, _lib.E_SPACE):
                _lib.check(rc, err)
            cap = int(n_pairs.value)
        arrs.update(row_ptr=row_ptr, n_pairs=int(n_pairs.value))
        if not emit:
            return arrs
        k, r, rd = np.empty(cap, np.int32), np.empty(cap, np.float64), np.empty(cap, np.float64)
        rc, err = call(k, r, rd, cap)
        arrs["n_pairs"] = int(n_pairs.value)
        _lib.check(rc, err)
        arrs.update(k=k[:arrs["n_pairs"]], r=r[:arrs["n_pairs"]], rd=rd[:arrs["n_pairs"]])
        return arrs

    def run_device(self, ld_wind, maf, std_thr, rsq_thr, positions, table, *, own=None, flags=0):
        """As `run`, but the owned slice of the score table stays on the device: `table` is a float64 device
        tensor of shape (7, width) on this engine's GPU (rows l2, l2d, maf, residuals_std, l2_ws, l2d_ws, l2d_wse;
        column c = SNP own[0] + c; NaN past the slice), written when this returns (C ABI nldsc_engine_run_device)."""
        n = self.n_snp
        own = (0, n) if own is None else own
        if table.dim() != 2 or table.shape[0] != 7 or not table.is_cuda or str(table.dtype) != "torch.float64" \
                or not table.is_contiguous():
            raise ValueError("table must be a contiguous float64 CUDA tensor of shape (7, width)")
        p, _keep = _lib.make_params(n, self.n_org, ld_wind, maf, std_thr, rsq_thr, positions, flags=flags)
        _torch_ready(table)
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_run_device(self._h, ctypes.byref(p), int(own[0]), int(own[1]),
                                                      ctypes.c_void_p(table.data_ptr()), int(table.shape[1]), err,
                                                      len(err)), err)
        return table

    def run_device_split(self, ld_wind, maf, std_thr, rsq_thr, positions, table, export, *, own, flags=0) -> int:
        """First half of a split run (C ABI nldsc_engine_run_device_split): the loaded slice is the owned SNPs
        [own[0], own[1]) and the right halo after them; computes the pairs whose lower SNP is owned and writes the
        halo's accumulator rows into `export` (contiguous int64 device tensor of >= 6 * halo elements).  Returns the
        number of halo SNPs exported; finish with run_device_finish."""
        n = self.n_snp
        if table.dim() != 2 or table.shape[0] != 7 or not table.is_cuda or str(table.dtype) != "torch.float64" \
                or not table.is_contiguous():
            raise ValueError("table must be a contiguous float64 CUDA tensor of shape (7, width)")
        if not export.is_cuda or str(export.dtype) != "torch.int64" or not export.is_contiguous():
            raise ValueError("export must be a contiguous int64 CUDA tensor")
        p, _keep = _lib.make_params(n, self.n_org, ld_wind, maf, std_thr, rsq_thr, positions, flags=flags)
        cnt = ctypes.c_int32(0)
        _torch_ready(table, export)
        err = _lib.errbuf()
        _lib.check(self._L.nldsc_engine_run_device_split(
            self._h, ctypes.byref(p), int(own[0]), int(own[1]), ctypes.c_void_p(table.data_ptr()),
            int(table.shape[1]), ctypes.c_void_p(export.data_ptr()), int(export.numel() // 6), ctypes.byref(cnt),
            err, len(err)), err)
        return int(cnt.value)

    def run_device_finish(self, imported=None, n: int = 0):
        """Second half: add the left neighbour's exported block (int64 device tensor laid out [6][n]) into the
        first n owned SNPs, finalize and write the table given to run_device_split."""
        err = _lib.errbuf()
        ptr = ctypes.c_void_p(imported.data_ptr()) if (imported is not None and n > 0) else None
        if ptr is not None:
            _torch_ready(imported)
        _lib.check(self._L.nldsc_engine_run_device_finish(self._h, ptr, int(n), err, len(err)), err)

    def timings(self) -> dict:
        ms = (ctypes.c_double * 6)()
        flop, issued, pairs = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        nl = ctypes.c_int32()
        self._L.nldsc_engine_timings(self._h, ms, ctypes.byref(flop), ctypes.byref(issued), ctypes.byref(pairs),
                                        ctypes.byref(nl))
        keys = ("count_ms", "stats_ms", "schedule_ms", "band_ms", "finalize_ms", "total_ms")
        d = {k: ms[i] for i, k in enumerate(keys)}
        d.update(flop_alg=flop.value, flop_issued=issued.value, pairs=pairs.value, band_items=nl.value)
        ex, ops = ctypes.c_int32(), ctypes.c_double()
        self._L.nldsc_engine_path(self._h, ctypes.byref(ex), ctypes.byref(ops))
        L = self._L  # (an older build loaded for A/B timing may lack the newer entry points)
        d.update(exact_i8=ex.value > 0, path={0: "f32", 1: "i8", 2: "f4"}[ex.value], ops_alg_i8=ops.value,
                 ksplit=L.nldsc_engine_ksplit(self._h) if hasattr(L, "nldsc_engine_ksplit") else 1,
                 band_kernel=(BAND_KERNELS.get(L.nldsc_engine_band_kernel(self._h), "?")
                              if hasattr(L, "nldsc_engine_band_kernel") else "?"),
                 band_round_items=(self._L.nldsc_engine_band_round_items(self._h)
                                   if hasattr(self._L, "nldsc_engine_band_round_items") else 0),
                 band_tail_ksplit=(self._L.nldsc_engine_band_tail_ksplit(self._h)
                                   if hasattr(self._L, "nldsc_engine_band_tail_ksplit") else 1),
                 result_direct=(self._L.nldsc_engine_result_direct(self._h)
                                if hasattr(self._L, "nldsc_engine_result_direct") else -1))
        cp = (ctypes.c_int32 * 3)()
        if hasattr(L, "nldsc_engine_band_pair_items"):
            L.nldsc_engine_band_pair_items(self._h, cp)
        d.update(band_pair_items=cp[0], band_pairs=cp[1], band_pair_rest=cp[2])
        return d


def calculate(bedfile: str, n_snp, n_org, ld_wind, maf, std_thr, rsq_thr, positions, *, flags=0, device=-1,
              keep=None, annot=None, covar=None, dom_dom=False) -> dict:
    """One-shot C-ABI call `nldsc_ld_calculate` (file -> GPU -> results); with `keep` (0-based .fam line numbers,
    strictly ascending; n_org stays the file's count) `nldsc_ld_calculate_keep`, on those individuals only; with
    `annot` ([n_snp, C]) `nldsc_ld_calculate_annot`, which adds "l2_annot" and "l2d_annot" ([n_snp, C]); with `covar`
    (an orthonormal basis, one row per individual the run uses) `nldsc_ld_calculate_covar`; with `dom_dom`
    `nldsc_ld_calculate_domdom`, which adds "l2dd" ([n_snp]), not together with `annot` or `covar`."""
    p, _pos = _lib.make_params(n_snp, n_org, ld_wind, maf, std_thr, rsq_thr, positions, bedfile=bedfile,
                               flags=flags, device=device)
    arrs, res = _lib.alloc_result(n_snp)
    err = _lib.errbuf()
    if dom_dom:
        if annot is not None or covar is not None:
            raise _lib.NLDSCError(
                _lib.E_ARG, "dom-dom scores with annotations, a pair table or covariates in one run are not supported")
        idx = None if keep is None or len(keep) == 0 else np.ascontiguousarray(keep, dtype=np.int32)
        arrs["l2dd"] = np.full(n_snp, np.nan)
        _lib.check(_lib.lib().nldsc_ld_calculate_domdom(
            ctypes.byref(p), None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx),
            ctypes.byref(res), arrs["l2dd"].ctypes.data, err, len(err)), err)
        return arrs
    if covar is not None:
        if annot is not None:
            raise _lib.NLDSCError(_lib.E_ARG, "covariates with annotations or a pair table in one run are not supported")
        idx = None if keep is None or len(keep) == 0 else np.ascontiguousarray(keep, dtype=np.int32)
        q = _lib.covar_basis_matrix(covar, n_org if idx is None else len(idx))
        _lib.check(_lib.lib().nldsc_ld_calculate_covar(
            ctypes.byref(p), None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx), q.ctypes.data,
            q.shape[0], ctypes.byref(res), err, len(err)), err)
        return arrs
    if annot is not None:
        a = _lib.annot_matrix(annot, n_snp)
        idx = None if keep is None or len(keep) == 0 else np.ascontiguousarray(keep, dtype=np.int32)
        for k in ("l2_annot", "l2d_annot"):
            arrs[k] = np.full((a.shape[0], n_snp), np.nan).T
        _lib.check(_lib.lib().nldsc_ld_calculate_annot(
            ctypes.byref(p), None if idx is None else idx.ctypes.data, 0 if idx is None else len(idx), a.ctypes.data,
            a.shape[0], ctypes.byref(res), arrs["l2_annot"].T.ctypes.data, arrs["l2d_annot"].T.ctypes.data, err,
            len(err)), err)
        return arrs
    if keep is None or len(keep) == 0:
        _lib.check(_lib.lib().nldsc_ld_calculate(ctypes.byref(p), ctypes.byref(res), err, len(err)), err)
    else:
        idx = np.ascontiguousarray(keep, dtype=np.int32)
        _lib.check(_lib.lib().nldsc_ld_calculate_keep(ctypes.byref(p), idx.ctypes.data, len(idx), ctypes.byref(res),
                                                      err, len(err)), err)
    return arrs


def device_count() -> int:
    return int(_lib.lib().nldsc_device_count())


def synth_bed_device(device: int, ptr: int, n_snp: int, n_org: int, thr: np.ndarray, rho: float = 0.9,
                     missing: float = 0.01, seed: int = 7):
    t = np.ascontiguousarray(thr, dtype=np.float32)
    err = _lib.errbuf()
    _lib.check(_lib.lib().nldsc_synth_bed_device(int(device), ctypes.c_void_p(ptr), n_snp, n_org,
                                                 t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), float(rho),
                                                 float(missing), int(seed), err, len(err)), err)
