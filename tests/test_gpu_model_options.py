"""The activation / mask options of the FastEnhancer constructor (models/fastenhancer/default/model.py:384-419) on the MI355X,
against goldens the reference itself produced with those options (tools/gen_golden.py: fe_b_relu_sig, fe_b_gelu_tanh, fe_t_lrelu,
fe_t_elu, fe_tk_gelutanh, fe_ln_elu).  The shipped library has no kernel for them: one side build (FE_BUILD_TAG, FE_LOCAL_DEF) compiles the
six option shapes with `--add-shape ...,act=..,mask=..`, and every GPU check runs in a fresh child process on that library
(FASTENHANCER_HIP_LIB), each under its own time limit.  After a child that ends abnormally no further child is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "modelopts"

# golden -> (the shipped test name whose yaml it starts from, the model_kwargs overrides (= tools/gen_golden.py), --add-shape spec)
OPTION_GOLDENS = {
    "fe_b_relu_sig": ("fe_b", {"activation": "ReLU", "mask": "sigmoid"}, "48,2,36,24,3,512,256,1,act=relu,mask=sigmoid"),
    "fe_b_gelu_tanh": ("fe_b", {"activation": "GELU", "activation_kwargs": {}, "mask": "tanh"}, "48,2,36,24,3,512,256,1,act=gelu,mask=tanh"),
    "fe_t_lrelu": ("fe_t", {"activation": "LeakyReLU", "activation_kwargs": {"negative_slope": 0.2, "inplace": True}},
                   "24,2,20,16,2,512,256,1,act=leaky_relu,mask=none"),
    "fe_t_elu": ("fe_t", {"activation": "ELU", "activation_kwargs": {"alpha": 1.0}, "mask": "sigmoid"}, "24,2,20,16,2,512,256,1,act=elu,mask=sigmoid"),
    "fe_tk_gelutanh": ("fe_tk_b", {"activation": "GELU", "activation_kwargs": {"approximate": "tanh"}, "mask": "sigmoid"},
                       "48,2,36,24,3,512,256,3,act=gelu_tanh,mask=sigmoid"),
    "fe_ln_elu": ("fe_ln_b", {"activation": "ELU", "activation_kwargs": {"alpha": 0.5}, "mask": "tanh"},
                  "48,2,36,24,3,512,256,1,0,0,0,1,act=elu,mask=tanh"),
}

_STATE = {"lib": None, "build_error": None, "crashed": None}


def _side_library(tmp_path_factory):
    """the side build, once per session: a failed build is recorded and fails the remaining tests without building again"""
    if _STATE["build_error"] is not None:
        pytest.fail(f"the side build of the option shapes failed earlier in this session: {_STATE['build_error']}")
    if _STATE["lib"] is None:
        local = tmp_path_factory.mktemp("model_options") / "local.def"
        env = dict(os.environ, FE_BUILD_TAG=TAG, FE_LOCAL_DEF=str(local))
        code = ("from fastenhancer_amd import build as b\n"
                f"for spec in {[v[2] for v in OPTION_GOLDENS.values()]!r}:\n"
                "    assert b.add_shape(spec), spec\n"
                "b.build()\n")
        try:
            r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=1500)
        except subprocess.TimeoutExpired:
            _STATE["build_error"] = "time limit (1500 s)"
            raise
        if r.returncode != 0:
            _STATE["build_error"] = f"exit status {r.returncode}"
        assert r.returncode == 0, r.stderr[-3000:]
        _STATE["lib"] = os.path.join(REPO, "ab", f"lib_{TAG}.so")
    return _STATE["lib"]


# what a child runs: the checks of one golden, printing "OK" at the end
CHILD = r'''
import json, sys
import numpy as np, torch
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import importlib
from common import MODEL_KWARGS, MODEL_MODULE, build_oracle, load_golden, rms
from oracle.fe_oracle import FEConfig as OCfg
from oracle.weightgen import make_input, make_training_state_dict
from fastenhancer_amd.streaming import StreamingModel, enhance_stream

ABS_TOL, REL_TOL, TIGHT = 1e-4, 1e-4, 2e-5          # tests/test_gpu_parity.py: the north_star bound and the fastenhancer family's regression bound

def close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    err, r = rms(got - ref), rms(ref)
    rel = err / max(r, 1e-3)
    assert err < ABS_TOL * max(1.0, r) and err <= REL_TOL * max(r, 1e-3), f"{what}: rms err {err:.3e}, ref rms {r:.3e}"
    assert rel <= TIGHT, f"{what}: relative rms err {rel:.3e} > {TIGHT:.0e}"
    print(f"{what}: rel {rel:.2e}")

dev = torch.device("cuda:0")
g = load_golden(NAME)
kw0, sr, _ = MODEL_KWARGS[BASE]
kw = json.loads(json.dumps(kw0)); kw.update(OVER)
variant = MODEL_MODULE[BASE]
seed = int(g["seed"])
ocfg = OCfg.from_model_kwargs(kw, variant=variant.split(".")[-1])
sd = {k: torch.from_numpy(np.asarray(v)) for k, v in make_training_state_dict(ocfg, seed).items()}
_, _, _, orc = build_oracle(BASE)               # (its STFT only: the same n_fft / hop / window)
mod = importlib.import_module(f"fastenhancer_amd.models.{variant}.model")
m = mod.ONNXModel(**kw).to(dev).eval(); m.load_state_dict(sd, strict=True)
cfg = m.engine.cfg
assert (cfg.activation, cfg.mask) != (0, 0)
B, hops, H = int(g["B"]), int(g["hops"]), cfg.hop_size

# streaming step over `hops` hops: waveform and caches
M = StreamingModel(m)
x = torch.from_numpy(make_input(B, hops * H, seed + 1000, sr)).to(dev)
caches = M.initialize_cache(x); outs = []
for t in range(hops):
    o, *caches = M(x[:, t * H:(t + 1) * H], *caches); outs.append(o.cpu().numpy())
close(np.stack(outs, 0), g["stream_wav_out"], "stream wav_out")
close(caches[0].cpu().numpy(), g["stream_cache_stft"], "cache_stft")
close(caches[1].cpu().numpy(), g["stream_cache_istft"], "cache_istft")
for k in range(len(caches) - 2):
    close(caches[2 + k].cpu().numpy(), g[f"stream_h{k}"], f"model cache {k}")
if NAME == "fe_b_relu_sig":
    assert m.engine.last_step_kernel().startswith("fe_frame8_kernel"), m.engine.last_step_kernel()

# the 200-hop driver loop (scripts/test_onnx.py): default per-hop kernel, the 256-thread kernel, 16-hop chunks bit-identical to it
if "long_wav_out" in g.files and not BASE.startswith(("fe_tk", "fe_ln")):
    length = int(g["long_length"])
    xl = torch.from_numpy(make_input(1, length, seed + 3000, sr))
    y1 = enhance_stream(m, xl, frames_per_call=1).cpu().numpy()
    close(y1[0], g["long_wav_out"], "long run T=1")
    m.engine.set_step_kernel("waves4")
    y1w = enhance_stream(m, xl, frames_per_call=1).cpu().numpy()
    y16 = enhance_stream(m, xl, frames_per_call=16).cpu().numpy()
    close(y1w[0], g["long_wav_out"], "long run T=1, 256-thread kernel")
    assert np.array_equal(y1w, y16), "chunked launches must be bit-identical to per-hop launches"
    m.engine.set_step_kernel("wg8")

# spec -> spec, a 4-frame chunk from zero caches
xs = make_input(B, hops * H, seed + 1000, sr)
c = orc.initialize_cache(B)[0]; specs = []
for t in range(4):
    s, c = orc.stft_step(xs[:, t * H:(t + 1) * H], c); specs.append(s)
spec = torch.from_numpy(np.concatenate(specs, axis=2)).to(dev)
spec_hat, *h = m(spec, *m.initialize_cache(spec))
close(spec_hat.cpu().numpy(), g["chunk_spec_out"], "chunk spec_hat")
close(h[-1].cpu().numpy(), g["chunk_h_last"], "chunk h_last")

# offline Model.forward on every engine the variant has; a ragged call of two lengths = each file's own call
mo = mod.Model(**kw).to(dev).eval(); mo.load_state_dict(sd, strict=True)
xo = torch.from_numpy(make_input(B, hops * H + 37, seed + 2000, sr)).to(dev)
runs = [("frame_walk", 0), ("frame_walk", -1)] + ([("time_batched", -1)] if variant == "fastenhancer.default" else [])
for engine, pipe in runs:
    mo.engine.set_offline_engine(engine); mo.engine.set_time_pipeline(pipe)
    w, s_ = mo(xo)
    close(w.cpu().numpy(), g["offline_wav"], f"offline wav ({engine}, pipeline {pipe})")
    close(s_.cpu().numpy(), g["offline_spec"], f"offline spec ({engine}, pipeline {pipe})")
    if engine == "time_batched":
        assert "tb_" in mo.engine.last_step_kernel(), mo.engine.last_step_kernel()
    parts = [xo[0], xo[1, :xo.shape[1] - 3 * H - 11]]
    wr, sr_ = mo.engine.offline_ragged(parts)
    for b, p in enumerate(parts):
        w1, s1 = mo.engine.offline(p[None])
        close(wr[b].cpu().numpy(), w1[0].cpu().numpy(), f"ragged wav {b} ({engine}, pipeline {pipe})")
        close(sr_[b].cpu().numpy(), s1[0].cpu().numpy(), f"ragged spec {b} ({engine}, pipeline {pipe})")

# many streams: the golden's streams tiled to 600 (more than #CUs: persistent workgroups of the plain kernel)
NS = 600
st = m.engine.new_state(NS)
xt = x[torch.arange(NS, device=dev) % B].contiguous()
outs = []
for t in range(hops):
    outs.append(m.engine.step(xt[:, t * H:(t + 1) * H].contiguous(), st).cpu().numpy())
got = np.stack(outs, 0)
for b in range(NS):
    close(got[:, b], g["stream_wav_out"][:, b % B], f"stream {b} of {NS}") if b < 4 or b % 97 == 0 or b == NS - 1 else None
ref = g["stream_wav_out"][:, np.arange(NS) % B]
close(got, ref, f"all {NS} streams")
print("OK")
'''


@pytest.mark.parametrize("name", list(OPTION_GOLDENS))
def test_model_options_match_reference_golden(name, tmp_path_factory):
    if _STATE["crashed"]:
        pytest.fail(f"not run: the child of {_STATE['crashed']} ended abnormally before it")
    lib = _side_library(tmp_path_factory)
    base, over, _ = OPTION_GOLDENS[name]
    code = f"REPO = {REPO!r}\nNAME = {name!r}\nBASE = {base!r}\nOVER = {over!r}\n" + CHILD
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FASTENHANCER_HIP_LIB=lib), capture_output=True, text=True,
                           timeout=600)
    except subprocess.TimeoutExpired:
        _STATE["crashed"] = name
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _STATE["crashed"] = name
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
