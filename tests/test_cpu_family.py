"""What the Python layer derives from a family's description, pinned to a fixture (no GPU) for every configuration name: the fe_config
bytes handed to fe_create, and (the noncausal models apart, which have no streaming state) where each tensor of the reference's cache
list lies inside the C ABI state (offset in floats, shape, stride of every tensor of Engine.split_state for a fresh state).  On top of the recorded geometry: pack_state inverts split_state, and
every streaming mirror's initialize_cache has the recorded shapes.

Regenerate (only when a layout is meant to change): python tests/test_cpu_family.py.  The generator calls only Engine.split_state,
state_floats and fe_create, so it also runs against an earlier revision of the package (how the fixture was first written: this file
and this revision's tests/common.py over the package of the commit before the family descriptions, its library built)."""
import contextlib
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":          # (run as a script, nothing has put the tests' and the repository's directories on the path)
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from common import CONFIG_NAMES, NONCAUSAL, hip_model, product_config

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "state_geometry.json")
BATCHES = (1, 3)
STREAMING = tuple(n for n in CONFIG_NAMES if n not in NONCAUSAL)      # (the noncausal module has the offline Model only: no state)


@contextlib.contextmanager
def fe_create_configs():
    """the bytes of every fe_config passed to fe_create inside the block"""
    from fastenhancer_amd import _lib
    lib, seen = _lib.load(), []
    real = lib.fe_create

    def fe_create(c, h):
        seen.append(bytes(c._obj))
        return real(c, h)
    lib.fe_create = fe_create
    try:
        yield seen
    finally:
        lib.fe_create = real


def make_engine(name):
    from fastenhancer_amd.engine import Engine
    with fe_create_configs() as seen:
        eng = Engine(product_config(name), None)
    (cfg_bytes,) = seen
    return eng, cfg_bytes


def numbered_state(eng, B):
    return torch.arange(eng.state_floats(B), dtype=torch.float32)


def state_geometry(name):
    eng, cfg_bytes = make_engine(name)
    out = {"fe_config": cfg_bytes.hex(), "split_state": {}}
    for B in BATCHES if name in STREAMING else ():
        views = eng.split_state(numbered_state(eng, B), B, head0=True)
        out["split_state"][str(B)] = [[t.storage_offset(), list(t.shape), list(t.stride())] for t in views]
    return out


def write_fixture():
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(state_geometry(n), sort_keys=True)}" for n in sorted(CONFIG_NAMES)) + "\n}\n")


def want(name):
    return json.load(open(FIXTURE))[name]


def test_the_fixture_covers_every_configuration_name():
    assert sorted(json.load(open(FIXTURE))) == sorted(CONFIG_NAMES)


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_fe_config_and_state_geometry_match_the_fixture(name):
    have = json.loads(json.dumps(state_geometry(name)))
    assert have["fe_config"] == want(name)["fe_config"], name
    assert set(have["split_state"]) == set(want(name)["split_state"]) == {str(B) for B in BATCHES if name in STREAMING}
    for B in have["split_state"]:
        assert have["split_state"][B] == want(name)["split_state"][B], (name, B)
    assert set(have) == set(want(name))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", STREAMING)
def test_pack_state_inverts_split_state(name, B):
    eng, _ = make_engine(name)
    s = numbered_state(eng, B)
    covered = sum(t.numel() for t in eng.split_state(s, B, head0=True))
    dpt = getattr(eng.cfg, "dpt", False)
    assert s.numel() - covered == (B if dpt else 0), (name, covered, s.numel())     # (the dptransformer ring heads follow the caches)
    s[covered:] = 0.0                # heads 0: the reference's oldest-first tensors are the rings themselves
    keep = s.clone()
    packed = eng.pack_state(eng.split_state(s, B), B)
    assert packed.dtype == torch.float32 and packed.shape == keep.shape
    assert torch.equal(packed.view(torch.int32), keep.view(torch.int32)), name
    assert torch.equal(s.view(torch.int32), keep.view(torch.int32)), name           # (the state itself is not written)


@pytest.mark.parametrize("name", STREAMING)
def test_mirror_initialize_cache_has_the_recorded_shapes(name):
    m = hip_model(name, load=False)
    for B in BATCHES:
        shapes = [tuple(shape) for _, shape, _ in want(name)["split_state"][str(B)]]
        caches = m.initialize_cache(torch.zeros(B, 1))
        assert [tuple(t.shape) for t in caches] == shapes[2:], (name, B)
        assert all(t.dtype == torch.float32 and t.device.type == "cpu" and not t.any() for t in caches)
        assert [tuple(t.shape) for t in m.stft.initialize_cache(torch.zeros(B, 1))] == shapes[:2], (name, B)


if __name__ == "__main__":
    write_fixture()
