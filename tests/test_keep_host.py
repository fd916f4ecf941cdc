"""--keep / --remove on the host side: the `FID IID` lists resolved to .fam line numbers, the whole-genome rule
(every chromosome's .fam must select the same individuals), the drop-in's `keep` attribute and the CLI flags.  No
GPU: the engine's own validation of an index list needs an engine (tests/test_gpu_keep.py)."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle as O


def write_fam(path, ids):
    with open(path, "w") as fh:
        for fid, iid in ids:
            fh.write(f"{fid}\t{iid}\t0\t0\t1\t-9\n")


@pytest.fixture()
def fam(tmp_path):
    from nldsc_amd.ldscore.common import FAMFile
    ids = [(f"F{i}", f"I{i}") for i in range(10)]
    write_fam(tmp_path / "a.fam", ids)
    return FAMFile(str(tmp_path / "a.fam")), ids


@pytest.fixture()
def warnings_of():
    """The `nldsc` logger's warnings (it does not propagate to the root logger)."""
    from nldsc_amd.core.logger import log
    seen = []

    class H(logging.Handler):
        def emit(self, rec):
            if rec.levelno >= logging.WARNING:
                seen.append(rec.getMessage())
    h = H()
    log.addHandler(h)
    yield seen
    log.removeHandler(h)


def test_fam_parses_fid_and_iid(fam, tmp_path):
    from nldsc_amd.ldscore.common import FAMFile
    f, ids = fam
    assert f.n_org == 10 and f.ids == ids
    # PLINK accepts spaces as well as tabs; blank lines are not individuals
    (tmp_path / "s.fam").write_text("A 1 0 0 1 -9\n\nB  2 0 0 2 -9\r\n")
    g = FAMFile(str(tmp_path / "s.fam"))
    assert g.n_org == 2 and g.ids == [("A", "1"), ("B", "2")]


def test_no_files_means_everyone(fam):
    from nldsc_amd.ldscore.common import kept_individuals
    assert kept_individuals(fam[0]) is None


def test_keep_follows_fam_order_and_collapses_duplicates(fam, tmp_path, warnings_of):
    from nldsc_amd.ldscore.common import kept_individuals
    (tmp_path / "k.txt").write_text("F7 I7\nF2 I2 extra columns ignored\n\nF7\tI7\n  F0   I0  \n")
    idx = kept_individuals(fam[0], keep=str(tmp_path / "k.txt"))
    assert idx.dtype == np.int32 and idx.tolist() == [0, 2, 7]
    assert warnings_of == []


def test_unknown_ids_are_counted_in_one_warning(fam, tmp_path, warnings_of):
    from nldsc_amd.ldscore.common import kept_individuals
    (tmp_path / "k.txt").write_text("F1 I1\nF1 I2\nX Y\nF3 I3\n")  # (F1, I2): FID and IID must both match
    idx = kept_individuals(fam[0], keep=str(tmp_path / "k.txt"))
    assert idx.tolist() == [1, 3]
    assert len(warnings_of) == 1 and "2 of 4" in warnings_of[0]


def test_remove_alone_and_keep_then_remove(fam, tmp_path):
    from nldsc_amd.ldscore.common import kept_individuals
    (tmp_path / "r.txt").write_text("F9 I9\nF0 I0\nF4 I4\n")
    assert kept_individuals(fam[0], remove=str(tmp_path / "r.txt")).tolist() == [1, 2, 3, 5, 6, 7, 8]
    (tmp_path / "k.txt").write_text("".join(f"F{i} I{i}\n" for i in (8, 4, 5, 0, 6)))
    assert kept_individuals(fam[0], keep=str(tmp_path / "k.txt"), remove=str(tmp_path / "r.txt")).tolist() == [5, 6, 8]


def test_empty_result_and_malformed_line_raise(fam, tmp_path):
    from nldsc_amd.ldscore.common import NLDSCParameterError, kept_individuals
    (tmp_path / "none.txt").write_text("X Y\n")
    with pytest.raises(NLDSCParameterError):
        kept_individuals(fam[0], keep=str(tmp_path / "none.txt"))
    (tmp_path / "all.txt").write_text("".join(f"F{i} I{i}\n" for i in range(10)))
    with pytest.raises(NLDSCParameterError):
        kept_individuals(fam[0], remove=str(tmp_path / "all.txt"))
    (tmp_path / "bad.txt").write_text("F1 I1\nF2\n")
    with pytest.raises(NLDSCParameterError):
        kept_individuals(fam[0], keep=str(tmp_path / "bad.txt"))
    with pytest.raises(NLDSCParameterError):
        kept_individuals(fam[0], remove=str(tmp_path / "bad.txt"))
    with pytest.raises(FileNotFoundError):
        kept_individuals(fam[0], keep=str(tmp_path / "missing.txt"))


@pytest.fixture()
def genome(tmp_path):
    from nldsc_amd import synth
    for i, c in enumerate((1, 2)):
        synth.write_plink(str(tmp_path / f"chr{c}"), synth.SynthSpec(n_org=41, n_snp=30, length_cm=0.5, seed=60 + i),
                          chrom=c)
    (tmp_path / "k.txt").write_text("".join(f"F{i} I{i}\n" for i in range(3, 41, 2)))
    return tmp_path


def test_genome_passes_the_same_list_to_every_chromosome(genome):
    """A caller's runner receives the index list; the run itself (here: the oracle on the host-subsetted rows, PLINK
    order) sees n_org of the file."""
    from nldsc_amd import synth
    from nldsc_amd.ldscore.genome import estimate_lds_genome
    seen = []

    def runner(bed, n_snp, n_org, w, maf, std_thr, rsq, pos, flags, keep=None):
        seen.append((n_org, None if keep is None else list(keep)))
        rows = np.asarray(bed[3:]).reshape(n_snp, -1)
        codes = O.unpack_codes(rows, n_org, strict=True)[:, keep]
        g = np.select([codes == 0, codes == 2, codes == 3], [0, 1, 2], -1).astype(np.int8)
        sub = synth.bed_bytes(synth.pack_bed_rows(g))
        return O.run_c(sub, n_snp, len(keep), w, maf, std_thr, rsq, pos, flags=O.STRICT_ORDER, threads=1), {}

    res = estimate_lds_genome(str(genome / "chr@"), "1", "cm", maf_thr="0.01", std_thr=1e-5, runner=runner, rank=0,
                              world=1, keep=str(genome / "k.txt"))
    assert sorted(res) == ["1", "2"]
    assert seen == [(41, list(range(3, 41, 2)))] * 2


def test_genome_fam_mismatch_raises(genome):
    from nldsc_amd.ldscore.common import NLDSCParameterError
    from nldsc_amd.ldscore.genome import estimate_lds_genome
    ids = [(f"F{i}", f"I{i}") for i in range(41)]
    ids[4], ids[5] = ids[5], ids[4]  # the same people on other lines: other bit pairs of the .bed rows
    write_fam(genome / "chr2.fam", ids)

    def runner(*a, **k):
        raise AssertionError("no chromosome may run")

    with pytest.raises(NLDSCParameterError, match="chr2.fam"):
        estimate_lds_genome(str(genome / "chr@"), "1", "cm", maf_thr="0.01", std_thr=1e-5, runner=runner, rank=0,
                            world=1, keep=str(genome / "k.txt"))


def test_pybind_params_keep_attribute():
    from nldsc_amd.ldscore import _ldscore as lds
    p = lds.LDScoreParams()
    assert p.keep == []
    p.keep = [0, 3, 7]
    assert p.keep == [0, 3, 7]
    q = lds.LDScoreParams("x.bed", n_snp=1, n_org=8, ld_wind=1.0, maf=0.0, std_thr=0.0, rsq_thr=0.0, positions=[0.0])
    assert q.keep == []
    q.keep = list(range(8))
    assert q.keep == list(range(8)) and q.n_org == 8
    q.keep = []
    assert q.keep == []


def test_cli_help_lists_keep_and_remove():
    p = subprocess.run([sys.executable, "-m", "nldsc_amd", "ld", "--help"], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--keep" in p.stdout and "--remove" in p.stdout
    assert "PLINK sample order" in " ".join(p.stdout.split())
