"""The fp8 KV cache option above the kernels, without a GPU: option parsing, the C ABI's refusal of unknown dtypes, the server flag, and the
checkpoint's self_attn.k_scale / v_scale tensors becoming cache scales instead of engine weights."""
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch

from dots_ocr_amd import engine as E
from dots_ocr_amd import modeling
from dots_ocr_amd.config import DotsConfig
from dots_ocr_amd.weights import random_state_dict, save_safetensors


def test_engine_rejects_a_bad_kv_cache_dtype_before_the_gpu(monkeypatch):
    def no_lib():
        raise AssertionError("the library / GPU was touched")
    monkeypatch.setattr(E._lib, "load", no_lib)
    for bad in ("fp16", "e5m2", "FP8", ""):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            E.Engine(DotsConfig.tiny(), kv_cache_dtype=bad)
    monkeypatch.setenv("DOTS_OCR_KV_CACHE_DTYPE", "int8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        E.Engine(DotsConfig.tiny())


def test_kv_cache_dtype_resolution_and_struct_field(monkeypatch):
    monkeypatch.delenv("DOTS_OCR_KV_CACHE_DTYPE", raising=False)
    assert E.resolve_kv_cache_dtype(None) == "bf16"
    monkeypatch.setenv("DOTS_OCR_KV_CACHE_DTYPE", "fp8")
    assert E.resolve_kv_cache_dtype(None) == "fp8"
    assert E.resolve_kv_cache_dtype("bf16") == "bf16"          # an explicit argument wins over the environment
    cc = E.c_config(DotsConfig.tiny(), 2, 256, 256, 256, kv_cache_dtype="fp8")
    assert cc.kv_cache_dtype == 1
    assert E.c_config(DotsConfig.tiny(), 2, 256, 256, 256).kv_cache_dtype == 0
    for sym in ("dots_set_kv_scales", "dots_debug_read_kv", "dots_op_dec_qkv_kv8", "dots_op_decode_attn_kv8"):
        assert sym in E.EXPORTED_SYMBOLS


def test_dots_create_refuses_an_unknown_kv_cache_dtype():
    """dots_create checks the config before it looks for a device."""
    lib = E._lib.load()
    E._prototypes(lib)
    cc = E.c_config(DotsConfig.tiny(), 2, 256, 256, 256)
    cc.kv_cache_dtype = 2
    h = C.c_void_p()
    assert lib.dots_create(C.byref(cc), 0, C.byref(h)) == -1
    assert b"kv_cache_dtype" in lib.dots_last_error(None)


def test_server_passes_kv_cache_dtype_to_the_model_factory(monkeypatch):
    from dots_ocr_amd import server
    seen = {}

    class Stop(Exception):
        pass

    def factory(name):
        def f(*a, **kw):
            seen[name] = kw
            raise Stop
        return f
    monkeypatch.setitem(sys.modules, "uvicorn", types.SimpleNamespace(run=lambda *a, **k: None))
    monkeypatch.setattr(modeling.DotsOcrHipForCausalLM, "from_random", factory("random"))
    monkeypatch.setattr(modeling.DotsOcrHipForCausalLM, "from_pretrained", factory("pretrained"))
    with pytest.raises(Stop):
        server.main(["--random-weights", "--kv-cache-dtype", "fp8"])
    assert seen["random"]["kv_cache_dtype"] == "fp8"
    with pytest.raises(Stop):
        server.main(["--model-path", "/nonexistent", "--kv-cache-dtype", "bf16"])
    assert seen["pretrained"]["kv_cache_dtype"] == "bf16"
    with pytest.raises(Stop):
        server.main(["--random-weights"])
    assert seen["random"]["kv_cache_dtype"] is None              # unset: the engine reads DOTS_OCR_KV_CACHE_DTYPE
    with pytest.raises(SystemExit):
        server.main(["--random-weights", "--kv-cache-dtype", "fp16"])


class FakeEngine:
    def __init__(self, cfg, **kw):
        self.kw, self.loaded, self.scales = kw, None, None

    def load_state_dict(self, sd):
        self.loaded = dict(sd)

    def set_kv_scales(self, s):
        self.scales = np.asarray(s)


def test_from_pretrained_turns_k_v_scale_tensors_into_cache_scales(monkeypatch, tmp_path):
    cfg = DotsConfig.tiny(layers=3, v_layers=2, vocab=1024)
    sd = random_state_dict(cfg, seed=1)
    sd["model.layers.0.self_attn.k_scale"] = torch.tensor([0.25])
    sd["model.layers.0.self_attn.v_scale"] = torch.tensor([0.5])
    sd["model.layers.2.self_attn.v_scale"] = torch.tensor([2.0])
    save_safetensors(sd, tmp_path / "model.safetensors")
    monkeypatch.setattr(modeling.DotsConfig, "from_pretrained", staticmethod(lambda p: cfg))
    monkeypatch.setattr(modeling, "Engine", FakeEngine)
    m = modeling.DotsOcrHipForCausalLM.from_pretrained(tmp_path, device=0, kv_cache_dtype="fp8")
    assert m.engine.kw["kv_cache_dtype"] == "fp8"
    assert not any(n.endswith(("k_scale", "v_scale")) for n in m.engine.loaded), "scale tensors were forwarded as weights"
    assert set(m.engine.loaded) == {n for n in sd if not n.endswith(("k_scale", "v_scale"))}
    want = np.ones((cfg.num_hidden_layers, cfg.num_key_value_heads, 2), np.float32)
    want[0, :, 0], want[0, :, 1], want[2, :, 1] = 0.25, 0.5, 2.0
    assert np.array_equal(m.engine.scales, want)
    # a checkpoint without scale tensors sets none (the engine keeps 1.0)
    m2 = modeling.DotsOcrHipForCausalLM(cfg, random_state_dict(cfg, seed=2), kv_cache_dtype=None)
    assert m2.engine.scales is None and m2.engine.kw["kv_cache_dtype"] is None
