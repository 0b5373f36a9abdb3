"""fastenhancer_amd/build.py decides from a translation unit's #include lines when its object is stale, and sizes its compiler pool
by MAX_JOBS.  No compiler runs here and no GPU is needed."""
import os
import shutil

import pytest

from fastenhancer_amd import build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join("..", "..", "include", "fastenhancer_hip.h")
# the dependency lists build.py kept by hand before it read them from the sources (relative to csrc/)
FE = ["fe_kernels.hip.h", "fe_launch.h", "fe_frame8.hip.h", "fe_impl.h", "tb_kernels.hip.h"]
BSRNN = ["fe_kernels.hip.h", "fe_launch.h", "bsrnn_kernels.hip.h", "bsrnn_sb_kernels.hip.h", "bsrnn_ov_kernels.hip.h"]
FSPEN = ["fe_kernels.hip.h", "fe_launch.h", "fspen_kernels.hip.h", "fspen_sb_kernels.hip.h"]
LISENNET = FSPEN + ["lisennet_kernels.hip.h", "lisennet_sb_kernels.hip.h"]
API = FE + BSRNN + LISENNET + ["fe_shapes.def", "fe_bsrnn_shapes.def", "stft_kernels.hip.h", "fe_api_bsrnn.inc", "fe_api_fspen.inc",
                               "fe_api_lisennet.inc", "fe_fragments.h", HEADER]
UNITS = {"fe_api.hip": API, "fe_shape.hip.in": FE, "fe_bsrnn_shape.hip.in": BSRNN, "fe_fspen.hip": FSPEN, "fe_lisennet.hip": LISENNET}


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_dependencies_cover_the_hand_kept_list_and_exist(unit):
    got = build.deps(os.path.join(build.CSRC, unit))
    assert len(got) == len(set(got)) and all(os.path.isabs(p) for p in got)
    missing = [d for d in UNITS[unit] + [unit, "fe_handover.h"] if os.path.normpath(os.path.join(build.CSRC, d)) not in got]
    assert not missing, missing
    assert all(os.path.isfile(p) for p in got), [p for p in got if not os.path.isfile(p)]


def test_a_new_header_under_fe_kernels_reaches_every_unit(tmp_path):
    csrc = tmp_path / "fastenhancer_amd" / "csrc"
    shutil.copytree(build.CSRC, csrc, ignore=shutil.ignore_patterns("_obj*"))
    shutil.copytree(os.path.join(REPO, "include"), tmp_path / "include")
    (csrc / "fe_new.h").write_text("#pragma once\n")
    with open(csrc / "fe_kernels.hip.h", "a") as f:
        f.write('#ifdef NEVER_DEFINED\n  #  include "fe_new.h"\n#endif\n')      # (both branches of an #ifdef count)
    for unit in UNITS:
        got = build.deps(str(csrc / unit))
        assert str(csrc / "fe_new.h") in got, unit
        assert all(p.startswith(str(tmp_path)) for p in got), unit       # nothing of the real tree: paths are relative to the including file
    assert str(tmp_path / "include" / "fastenhancer_hip.h") in build.deps(str(csrc / "fe_api.hip"))


def test_pool_size_respects_max_jobs(monkeypatch):
    monkeypatch.setenv("MAX_JOBS", "3")
    assert build.pool_size(40) == 3 and build.pool_size(2) == 2
    monkeypatch.delenv("MAX_JOBS")
    assert build.pool_size(40) == min(40, os.cpu_count() or 2) and build.pool_size(0) == 1
