"""The weight packing on the CPU (fe_debug_pack_weights / Engine.pack_blob: what fe_load_weights runs between its two copies) and the
fragment orders of csrc/fe_fragments.h, checked by a stand-alone program against their written definition.  No GPU needed."""
import concurrent.futures
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

from fastenhancer_amd import _lib
from fastenhancer_amd.engine import Engine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
from packed_digests import configurations  # noqa: E402

CONFIGS = configurations()
FE_ERR_INVALID_ARG = -1      # include/fastenhancer_hip.h


def test_fragment_orders_against_their_definition(tmp_path):
    """tests/host/frag_check.cpp includes only the header; built with the host compiler and, where its runtime is installed,
    -fsanitize=address,undefined (a stand-alone program: nothing is preloaded)"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "frag_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(REPO, "fastenhancer_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "frag_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # the sanitizer runtime linked into the program where the compiler can (it then does not care what else the process loads first);
    # no sanitizer runtime for this compiler at all: the plain build must do
    for flags in (san + ["-static-libasan", "-static-libubsan"], san, []):
        if subprocess.run(cmd + flags, capture_output=True).returncode == 0:
            break
    else:
        pytest.fail(subprocess.run(cmd, capture_output=True, text=True).stderr[-3000:])
    print("frag_check built with", flags or "no sanitizer")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "frag_check: ok" in r.stdout, r.stdout + r.stderr


def _pack(eng, blob, out=None):
    """fe_debug_pack_weights into `out` (allocated from the size query when None) -> (rc, packed floats reported, out)"""
    n = ctypes.c_size_t(0)
    if out is None:
        assert eng.lib.fe_debug_pack_weights(eng._h, blob.data_ptr(), blob.numel(), None, 0, ctypes.byref(n)) == _lib.FE_OK
        out = torch.empty(n.value, dtype=torch.float32)
    rc = eng.lib.fe_debug_pack_weights(eng._h, blob.data_ptr(), blob.numel(), out.data_ptr(), out.numel(), ctypes.byref(n))
    return rc, n.value, out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_pack_blob_on_the_cpu(name):
    cfg, default_sd = CONFIGS[name]
    eng, eng2 = Engine(cfg, None), Engine(cfg, None)
    blob = eng.make_blob(default_sd(cfg, torch.Generator().manual_seed(7)))
    rc, n, packed = _pack(eng, blob)
    assert rc == _lib.FE_OK and n == packed.numel() > 0
    assert bool(torch.isfinite(packed).all())
    assert torch.equal(packed.view(torch.int32), eng2.pack_blob(blob).view(torch.int32))      # two fresh handles: the same bytes
    # the argument errors: FE_ERR_INVALID_ARG, nothing written
    out = torch.full((n,), 12345.0)
    cnt = ctypes.c_size_t(77)
    h, lib, p = eng._h, eng.lib, blob.data_ptr()
    for args in ((None, p, blob.numel(), out.data_ptr(), n), (h, None, blob.numel(), out.data_ptr(), n),
                 (h, p, blob.numel() - 1, out.data_ptr(), n), (h, p, blob.numel() + 4, out.data_ptr(), n), (h, p, blob.numel(), out.data_ptr(), n - 1)):
        assert lib.fe_debug_pack_weights(*args, ctypes.byref(cnt)) == FE_ERR_INVALID_ARG, args
        assert cnt.value == 77 and bool((out == 12345.0).all())
    assert lib.fe_last_error()


SENSITIVITY = ("fe_b", "fe_tk_b", "fe_ln_b", "fe_dpt_b", "fe_dprnn_b", "fe_nc", "bsrnn_xt", "bsrnn_s", "fspen", "lisennet")


@pytest.mark.parametrize("name", SENSITIVITY)
def test_every_weight_section_reaches_the_packed_buffer(name):
    """one section random, all others zero: the packed buffer differs from the all-zero blob's, for every section (a packer that
    drops or mis-addresses a section's reads cannot pass; the per-stage parity tests on the GPU check the values).  No section is
    exempt: with the packers as they were before csrc/fe_fragments.h every section of these ten models changed the buffer."""
    cfg = CONFIGS[name][0]
    first = Engine(cfg, None)
    zero_blob = torch.zeros(first.weight_floats)
    base = _pack(first, zero_blob)[2]
    rnd = torch.rand(first.weight_floats, generator=torch.Generator().manual_seed(5)) + 0.5      # (no zeros, no cancelling signs)
    workers = max(1, min(8, os.cpu_count() or 1))
    engines = [first] + [Engine(cfg, None) for _ in range(workers - 1)]      # a handle per thread: packing writes the handle's offset tables

    def unchanged(w):
        out = torch.empty_like(base)
        dead = []
        for sname, off, cnt in first.sections[w::workers]:
            blob = torch.zeros_like(zero_blob)
            blob[off:off + cnt] = rnd[off:off + cnt]
            rc, _, _ = _pack(engines[w], blob, out)
            assert rc == _lib.FE_OK
            if torch.equal(out, base):
                dead.append(sname)
        return dead

    with concurrent.futures.ThreadPoolExecutor(workers) as ex:
        dead = sorted(s for part in ex.map(unchanged, range(workers)) for s in part)
    assert dead == [], f"{name}: sections that do not reach the packed buffer"
