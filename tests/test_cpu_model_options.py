"""The model_kwargs options beyond the shipped yamls - the conv trunk's activation and the mask function
(models/fastenhancer/default/model.py:384-419) - on the host side: config parsing, the C ABI struct, the
`--add-shape` options and fe_create's answer for an option set that is not compiled.  No GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from common import MODEL_KWARGS
from fastenhancer_amd import _lib
from fastenhancer_amd import build as fbuild
from fastenhancer_amd.config import FEConfig, dprnn_config, dpt_config, ln_config, noncausal_config, time_kernel_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fastenhancer_hip.h")


def _kw(name="fe_b", **over):
    kw = dict(MODEL_KWARGS[name][0])
    kw.update(over)
    return kw


@pytest.mark.parametrize("activation, kwargs, code, param", [
    ("SiLU", {"inplace": True}, 0, 0.0),
    ("ReLU", {"inplace": True}, 1, 0.0),
    ("ReLU", None, 1, 0.0),
    ("LeakyReLU", {}, 2, 0.01),
    ("LeakyReLU", {"negative_slope": 0.2, "inplace": True}, 2, 0.2),
    ("ELU", {}, 3, 1.0),
    ("ELU", {"alpha": 0.5}, 3, 0.5),
    ("GELU", {}, 4, 0.0),
    ("GELU", {"approximate": "none"}, 4, 0.0),
    ("GELU", {"approximate": "tanh"}, 5, 0.0),
])
def test_config_accepts_the_supported_activations(activation, kwargs, code, param):
    cfg = FEConfig.from_model_kwargs(**_kw(activation=activation, activation_kwargs=kwargs))
    assert cfg.activation == code
    assert cfg.activation_param == pytest.approx(param)


def test_the_reference_default_activation_is_relu():
    kw = _kw()
    kw.pop("activation")
    kw.pop("activation_kwargs")
    assert FEConfig.from_model_kwargs(**kw).activation == _lib.FE_ACT_RELU


@pytest.mark.parametrize("mask, code", [(None, 0), ("sigmoid", 1), ("tanh", 2)])
def test_config_accepts_the_masks(mask, code):
    assert FEConfig.from_model_kwargs(**_kw(mask=mask)).mask == code


def test_config_refuses_what_it_does_not_build():
    with pytest.raises(RuntimeError, match=r"activation=PReLU is not supported.*supported: SiLU, ReLU, LeakyReLU\(negative_slope\), ELU\(alpha\), GELU"):
        FEConfig.from_model_kwargs(**_kw(activation="PReLU", activation_kwargs={}))
    with pytest.raises(RuntimeError, match=r"activation_kwargs \['beta'\] of SiLU are not supported.*supported: SiLU"):
        FEConfig.from_model_kwargs(**_kw(activation_kwargs={"beta": 2.0}))
    with pytest.raises(RuntimeError, match=r"activation_kwargs \['alpha'\] of LeakyReLU"):
        FEConfig.from_model_kwargs(**_kw(activation="LeakyReLU", activation_kwargs={"alpha": 2.0}))
    with pytest.raises(RuntimeError, match="approximate='fast'"):
        FEConfig.from_model_kwargs(**_kw(activation="GELU", activation_kwargs={"approximate": "fast"}))
    with pytest.raises(RuntimeError, match=r"mask=softmax is not supported\. \(supported: null, 'sigmoid', 'tanh'\)"):
        FEConfig.from_model_kwargs(**_kw(mask="softmax"))
    with pytest.raises(RuntimeError, match="resnet=True is not supported"):
        FEConfig.from_model_kwargs(**_kw(resnet=True))
    for flag in ("post_act", "pre_norm", "attn_bias"):
        with pytest.raises(RuntimeError, match=f"rnnformer_kwargs.{flag}=True"):
            FEConfig.from_model_kwargs(**_kw(rnnformer_kwargs=dict(_kw()["rnnformer_kwargs"], **{flag: True})))
    with pytest.raises(RuntimeError, match="window"):
        FEConfig.from_model_kwargs(**_kw(window="povey"))


def test_variants_take_the_options_where_built():
    tk = time_kernel_config(**_kw("fe_tk_b", activation="GELU", activation_kwargs={"approximate": "tanh"}, mask="sigmoid"))
    assert (tk.activation, tk.mask, tk.kernel_size_time) == (5, 1, 3)
    ln = ln_config(**_kw("fe_ln_b", activation="ELU", activation_kwargs={"alpha": 0.5}, mask="tanh"))
    assert (ln.activation, ln.activation_param, ln.mask, ln.ln) == (3, 0.5, 2, True)
    # no golden test of the options for these: they keep refusing them
    with pytest.raises(RuntimeError, match="dprnn variant"):
        dprnn_config(**_kw("fe_dprnn_b", activation="ReLU"))
    with pytest.raises(RuntimeError, match="dptransformer variant"):
        dpt_config(**_kw("fe_dpt_b", mask="sigmoid"))
    with pytest.raises(RuntimeError, match="noncausal variant"):
        noncausal_config(**_kw("fe_nc", activation="ReLU"))
    # the reference's time_kernel and dprnn constructors have no resnet argument
    with pytest.raises(TypeError):
        time_kernel_config(**_kw("fe_tk_b", resnet=True))
    with pytest.raises(TypeError):
        dprnn_config(**_kw("fe_dprnn_b", resnet=True))


def _struct_from_header():
    """the fields of `typedef struct fe_config` in the header, in order: (name, 'int' | 'float', count)"""
    src = open(HEADER).read()
    body = re.search(r"typedef struct fe_config \{(.*?)\} fe_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for nm in names.split(","):
            nm = nm.strip()
            m = re.match(r"(\w+)\[(\w+)\]", nm)
            fields.append((m.group(1), typ, _lib.FE_MAX_KERNELS) if m else (nm, typ, 1))
    return fields


def _c_offsets(tmp_path, names):
    """offsetof / sizeof from a C compiler, or None when there is none"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or next(
        (p for p in ("/opt/rocm/llvm/bin/clang",) if os.path.exists(p)), None)
    if cc is None:
        return None
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fastenhancer_hip.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %zu\\n", offsetof(fe_config, {n}));\n' for n in names)
                   + '    printf("sizeof %zu\\n", sizeof(fe_config));\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_ctypes_config_matches_the_header(tmp_path):
    fields = _struct_from_header()
    ct = _lib.fe_config._fields_
    assert [f[0] for f in fields] == [f[0] for f in ct]
    for (name, typ, n), (cname, ctyp) in zip(fields, ct):
        base = ctypes.c_float if typ == "float" else ctypes.c_int
        assert ctyp == (base * n if n > 1 else base), name
    assert [f[0] for f in fields][-4:] == ["activation", "activation_param", "mask", "resnet"]
    c = _c_offsets(tmp_path, [f[0] for f in fields])
    if c is not None:
        for name, _, _ in fields:
            assert getattr(_lib.fe_config, name).offset == c[name], name
        assert ctypes.sizeof(_lib.fe_config) == c["sizeof"]
    defs = dict(re.findall(r"#define (FE_(?:ACT|MASK)_\w+) (\d+)", open(HEADER).read()))
    for k, v in defs.items():
        assert getattr(_lib, k) == int(v), k
    assert len(defs) == 9


def test_add_shape_parses_the_options(tmp_path, monkeypatch):
    assert fbuild.parse_shape_spec("48,2,36,24,3,512,256") == ([48, 2, 36, 24, 3, 512, 256], 0)
    assert fbuild.parse_shape_spec("48,2,36,24,3,512,256,1,act=relu,mask=sigmoid,resnet=0") == ([48, 2, 36, 24, 3, 512, 256, 1], 1 + 8)
    assert fbuild.parse_shape_spec("48,2,36,24,3,512,256,3,act=gelu_tanh")[1] == 5
    assert fbuild.parse_shape_spec("24,2,20,16,2,512,256,mask=tanh")[1] == 16
    local = tmp_path / "local.def"
    monkeypatch.setattr(fbuild, "LOCAL_DEF", str(local))
    a = fbuild.add_shape("48,2,36,24,3,512,256,1,act=relu,mask=sigmoid")
    b = fbuild.add_shape("48,2,36,24,3,512,256,1,act=gelu,mask=tanh")
    c = fbuild.add_shape("48,2,36,24,3,512,256,1,0,0,0,1,act=elu,mask=tanh")
    assert len({a, b, c}) == 3 and all(a)
    assert fbuild.add_shape("48,2,36,24,3,512,256,act=relu,mask=sigmoid") == ""        # the same option set: already listed
    lines = [ln for ln in local.read_text().splitlines() if ln.startswith("X(")]
    assert lines[0] == f"X({a}, 48, 2, 36, 24, 3, 512, 256, 1, 0, 0, 0, 0, 0, 9)"
    assert lines[2] == f"X({c}, 48, 2, 36, 24, 3, 512, 256, 1, 0, 0, 0, 1, 0, 19)"
    assert len(lines) == 3
    for bad, msg in [("48,2,36,24,3,512,256,act=swish", "act=swish is not supported"),
                     ("48,2,36,24,3,512,256,mask=softmax", "mask=softmax is not supported"),
                     ("48,2,36,24,3,512,256,resnet=1", "resnet=1 is not built"),
                     ("48,2,36,24,3,512,256,colour=red", "unknown option 'colour'"),
                     ("48,2,36,24,3,512,256,act=relu,act=elu", "given twice"),
                     ("48,act=relu,2,36,24,3,512,256", "come after the shape's numbers"),
                     ("48,2,36,24,3,512,x", "'x' is not an integer"),
                     ("48,2,36,24,3,512,256,1,0,1,act=relu", "default, time_kernel and ln models")]:
        with pytest.raises(SystemExit, match=msg):
            fbuild.add_shape(bad)
    assert len([ln for ln in local.read_text().splitlines() if ln.startswith("X(")]) == 3


def _create(cfg):
    lib = _lib.load()
    c = _lib.fe_config()
    c.arch = _lib.FE_ARCH_FASTENHANCER
    c.n_fft, c.hop_size, c.win_size, c.input_compression = cfg.n_fft, cfg.hop_size, cfg.win_size, cfg.input_compression
    c.channels, c.n_kernels, c.stride = cfg.channels, len(cfg.kernel_size), cfg.stride
    for i, k in enumerate(cfg.kernel_size):
        c.kernel_size[i] = k
    c.rf_channels, c.rf_freq, c.rf_blocks, c.rf_heads = cfg.rf_channels, cfg.rf_freq, cfg.rf_blocks, cfg.rf_heads
    c.kernel_size_time, c.ln, c.rf_eps = cfg.kernel_size_time, 1 if cfg.ln else 0, cfg.rf_eps
    c.activation, c.activation_param, c.mask = cfg.activation, cfg.activation_param, cfg.mask
    h = ctypes.c_void_p()
    rc = lib.fe_create(ctypes.byref(c), ctypes.byref(h))
    msg = lib.fe_last_error().decode()
    if rc == _lib.FE_OK:
        lib.fe_destroy(h)
    return rc, msg, c


@pytest.mark.parametrize("name, cfg_fn, over, cmd", [
    ("fe_b", FEConfig.from_model_kwargs, dict(activation="ReLU", mask="sigmoid"), "48,2,36,24,3,512,256,1,act=relu,mask=sigmoid"),
    ("fe_t", FEConfig.from_model_kwargs, dict(activation="LeakyReLU", activation_kwargs={"negative_slope": 0.2}),
     "24,2,20,16,2,512,256,1,act=leaky_relu,mask=none"),
    ("fe_tk_b", time_kernel_config, dict(activation="GELU", activation_kwargs={"approximate": "tanh"}, mask="sigmoid"),
     "48,2,36,24,3,512,256,3,act=gelu_tanh,mask=sigmoid"),
    ("fe_ln_b", ln_config, dict(activation="ELU", activation_kwargs={"alpha": 0.5}, mask="tanh"), "48,2,36,24,3,512,256,1,0,0,0,1,act=elu,mask=tanh"),
])
def test_fe_create_names_the_build_command_of_an_option_set(name, cfg_fn, over, cmd):
    """fe_create needs no GPU: the shipped library has no kernel for these options, and its message is the command that builds one"""
    cfg = cfg_fn(**_kw(name, **over))
    rc, msg, _ = _create(cfg)
    assert rc == -2, (rc, msg)                      # FE_ERR_UNSUPPORTED_CONFIG
    assert f"python -m fastenhancer_amd.build --add-shape {cmd})" in msg, msg
    assert cfg.options in msg
    ints, ep = fbuild.parse_shape_spec(cmd)        # the command, run as printed, builds this option set
    assert ep == cfg.activation + 8 * cfg.mask
    base = cfg_fn(**_kw(name))                     # ... and the shipped setting of the same shape is compiled
    assert _create(base)[0] == _lib.FE_OK


def test_fe_create_refuses_resnet_and_bad_codes():
    cfg = FEConfig.from_model_kwargs(**_kw())
    lib = _lib.load()
    _, _, c = _create(cfg)
    h = ctypes.c_void_p()
    c.resnet = 1
    assert lib.fe_create(ctypes.byref(c), ctypes.byref(h)) == -2 and "resnet" in lib.fe_last_error().decode()
    c.resnet, c.activation = 0, 6
    assert lib.fe_create(ctypes.byref(c), ctypes.byref(h)) == -1 and "activation=6" in lib.fe_last_error().decode()
    c.activation, c.mask = 0, 3
    assert lib.fe_create(ctypes.byref(c), ctypes.byref(h)) == -1 and "mask=3" in lib.fe_last_error().decode()
    c.mask, c.activation, c.channels_frnn = 0, 1, cfg.rf_channels // 2
    assert lib.fe_create(ctypes.byref(c), ctypes.byref(h)) == -2 and "dprnn variant" in lib.fe_last_error().decode()
