// ldscore_py.cpp — pybind11 module `_ldscore`, the drop-in for bayarpark/nldsc's extension of the
// same name (nldsc/ldscore/_ldscore/ldscore.cpp:17-54, stub nldsc/ldscore/_ldscore.pyi:1-25).
//
// Same classes, constructor signatures (keyword-only after `bfile`), read-write attributes and
// `calculate(params) -> LDScoreResult`; the work is done by libnldsc_amd.so through the C ABI
// in include/nldsc_ld.h, on the GPU.  There is no CPU fallback: without a HIP device
// `calculate` raises RuntimeError.
//
// Differences from the reference, all additive: the GIL is released during `calculate`;
// LDScoreParams has four extra attributes, `flags` (NLDSC_FLAG_*), `device` (HIP ordinal,
// default from $NLDSC_DEVICE, else the current device), `keep` (0-based .fam line numbers of the
// individuals to use, strictly ascending; empty: everyone — nldsc_ld_calculate_keep) and `annot` (an
// annotation matrix, row-major [n_snp][n_annot]; empty: none — nldsc_ld_calculate_annot), and
// LDScoreResult two, `l2_annot` and `l2d_annot` (row-major [n_snp][n_annot], empty without `annot`);
// LDScoreParams `dom_dom` (dominance-by-dominance LD scores — nldsc_ld_calculate_domdom; not with `annot`) fills
// LDScoreResult `l2dd` ([n_snp], empty without it); errors carry the engine's message.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/nldsc_ld.h"

namespace py = pybind11;

namespace {

struct LDScoreParams {  // data.h:33-65
    std::string bedfile;
    int n_snp = 0;
    int n_org = 0;
    double ld_wind = 0;
    std::vector<double> positions;
    double maf = 0;
    double std_thr = 0;
    double rsq_thr = 0;
    unsigned flags = 0;
    int device = -1;
    std::vector<int> keep;  // .fam lines of the individuals to use (empty: everyone); n_org stays the file's count
    std::vector<double> annot;  // annotation matrix, row-major [n_snp][n_annot] (empty: none)
    bool dom_dom = false;       // also the dominance-by-dominance scores (LDScoreResult::l2dd)

    LDScoreParams() {
        if (const char* d = std::getenv("NLDSC_DEVICE")) device = std::atoi(d);
    }
    LDScoreParams(const std::string& bfile, int n_snp_, int n_org_, double ld_wind_, double maf_, double std_thr_,
                  double rsq_thr_, const std::vector<double>& positions_)
        : LDScoreParams() {
        bedfile = bfile;
        n_snp = n_snp_;
        n_org = n_org_;
        ld_wind = ld_wind_;
        maf = maf_;
        std_thr = std_thr_;
        rsq_thr = rsq_thr_;
        positions = positions_;
    }
};

struct LDScoreResult {  // data.h:21-31
    std::vector<double> l2, l2d, maf, residuals_std;
    std::vector<int> l2_ws, l2d_ws, l2d_wse;
    std::vector<double> l2_annot, l2d_annot;  // row-major [n_snp][n_annot]; empty without LDScoreParams::annot
    std::vector<double> l2dd;                 // [n_snp]; empty without LDScoreParams::dom_dom
};

LDScoreResult calculate(const LDScoreParams& params) {
    if (params.n_snp < 0 || (size_t)params.n_snp != params.positions.size())
        throw std::invalid_argument("positions must have n_snp elements");
    LDScoreResult res;
    const size_t n = (size_t)std::max(params.n_snp, 0);
    res.l2.assign(n, 0.0);
    res.l2d.assign(n, 0.0);
    res.maf.assign(n, 0.0);
    res.residuals_std.assign(n, 0.0);
    res.l2_ws.assign(n, 0);
    res.l2d_ws.assign(n, 0);
    res.l2d_wse.assign(n, 0);
    nldsc_ld_params p{};
    p.bedfile = params.bedfile.c_str();
    p.n_snp = params.n_snp;
    p.n_org = params.n_org;
    p.ld_wind = params.ld_wind;
    p.positions = params.positions.data();
    p.maf = params.maf;
    p.std_thr = params.std_thr;
    p.rsq_thr = params.rsq_thr;
    p.flags = params.flags;
    p.device = params.device;
    nldsc_ld_result r{res.l2.data(), res.l2d.data(), res.maf.data(), res.residuals_std.data(),
                      reinterpret_cast<int32_t*>(res.l2_ws.data()), reinterpret_cast<int32_t*>(res.l2d_ws.data()),
                      reinterpret_cast<int32_t*>(res.l2d_wse.data())};
    char err[1024] = {0};
    int rc;
    if (params.dom_dom) {
        if (!params.annot.empty())
            throw std::invalid_argument(
                "dom-dom scores with annotations, a pair table or covariates in one run are not supported");
        std::vector<double> dd(n, 0.0);
        {
            py::gil_scoped_release nogil;
            rc = nldsc_ld_calculate_domdom(&p, params.keep.empty() ? nullptr
                                                                   : reinterpret_cast<const int32_t*>(params.keep.data()),
                                           (int32_t)params.keep.size(), &r, dd.data(), err, sizeof(err));
        }
        if (rc == NLDSC_OK) res.l2dd = std::move(dd);
    } else if (!params.annot.empty()) {
        if (n == 0 || params.annot.size() % n != 0)
            throw std::invalid_argument("annot must have n_snp * n_annot elements");
        const size_t C = params.annot.size() / n;
        // the C ABI takes and fills category-major [n_annot][n_snp] arrays
        std::vector<double> a(C * n), l2c(C * n), l2dc(C * n);
        for (size_t j = 0; j < n; ++j)
            for (size_t c = 0; c < C; ++c) a[c * n + j] = params.annot[j * C + c];
        {
            py::gil_scoped_release nogil;
            rc = nldsc_ld_calculate_annot(&p, params.keep.empty() ? nullptr
                                                                  : reinterpret_cast<const int32_t*>(params.keep.data()),
                                          (int32_t)params.keep.size(), a.data(), (int32_t)C, &r, l2c.data(), l2dc.data(),
                                          err, sizeof(err));
        }
        if (rc == NLDSC_OK) {
            res.l2_annot.resize(C * n);
            res.l2d_annot.resize(C * n);
            for (size_t j = 0; j < n; ++j)
                for (size_t c = 0; c < C; ++c) {
                    res.l2_annot[j * C + c] = l2c[c * n + j];
                    res.l2d_annot[j * C + c] = l2dc[c * n + j];
                }
        }
    } else {
        py::gil_scoped_release nogil;
        rc = params.keep.empty() ? nldsc_ld_calculate(&p, &r, err, sizeof(err))
                                 : nldsc_ld_calculate_keep(&p, reinterpret_cast<const int32_t*>(params.keep.data()),
                                                           (int32_t)params.keep.size(), &r, err, sizeof(err));
    }
    if (rc == NLDSC_E_BAD_MAGIC) throw std::invalid_argument(err);  // -> ValueError, as the reference
    if (rc != NLDSC_OK) throw std::runtime_error(err);
    return res;
}

}  // namespace

PYBIND11_MODULE(_ldscore, m) {
    static_assert(sizeof(int) == sizeof(int32_t), "int must be 32-bit");
    py::class_<LDScoreParams> P(m, "LDScoreParams");
    P.def(py::init());
    P.def(py::init<const std::string&, int, int, double, double, double, double, const std::vector<double>&>(),
          py::arg("bfile"), py::kw_only(), py::arg("n_snp"), py::arg("n_org"), py::arg("ld_wind"), py::arg("maf"),
          py::arg("std_thr"), py::arg("rsq_thr"), py::arg("positions"));
    P.def_readwrite("bedfile", &LDScoreParams::bedfile)
        .def_readwrite("n_snp", &LDScoreParams::n_snp)
        .def_readwrite("n_org", &LDScoreParams::n_org)
        .def_readwrite("ld_wind", &LDScoreParams::ld_wind)
        .def_readwrite("positions", &LDScoreParams::positions)
        .def_readwrite("maf", &LDScoreParams::maf)
        .def_readwrite("std_thr", &LDScoreParams::std_thr)
        .def_readwrite("rsq_thr", &LDScoreParams::rsq_thr)
        .def_readwrite("flags", &LDScoreParams::flags)
        .def_readwrite("device", &LDScoreParams::device)
        .def_readwrite("keep", &LDScoreParams::keep)
        .def_readwrite("annot", &LDScoreParams::annot)
        .def_readwrite("dom_dom", &LDScoreParams::dom_dom);

    py::class_<LDScoreResult> R(m, "LDScoreResult");
    R.def(py::init());
    R.def_readwrite("l2", &LDScoreResult::l2)
        .def_readwrite("l2d", &LDScoreResult::l2d)
        .def_readwrite("maf", &LDScoreResult::maf)
        .def_readwrite("residuals_std", &LDScoreResult::residuals_std)
        .def_readwrite("l2_ws", &LDScoreResult::l2_ws)
        .def_readwrite("l2d_ws", &LDScoreResult::l2d_ws)
        .def_readwrite("l2d_wse", &LDScoreResult::l2d_wse)
        .def_readwrite("l2_annot", &LDScoreResult::l2_annot)
        .def_readwrite("l2d_annot", &LDScoreResult::l2d_annot)
        .def_readwrite("l2dd", &LDScoreResult::l2dd);

    m.def("calculate", &calculate);
    m.attr("__version__") = nldsc_version();
    m.attr("FLAG_STRICT_PLINK_ORDER") = NLDSC_FLAG_STRICT_PLINK_ORDER;
    m.attr("FLAG_ADDITIVE_ONLY") = NLDSC_FLAG_ADDITIVE_ONLY;
    m.attr("FLAG_EXACT_I8") = NLDSC_FLAG_EXACT_I8;
    m.attr("FLAG_FP32") = NLDSC_FLAG_FP32;
    m.attr("FLAG_EXACT_F4") = NLDSC_FLAG_EXACT_F4;
    m.attr("FLAG_EXACT_RARE") = NLDSC_FLAG_EXACT_RARE;
}
