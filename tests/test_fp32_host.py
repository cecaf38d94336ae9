"""Host-side checks of the fp32 (reference precision, inference only) surface: no GPU needed."""
import re
import subprocess
import sys
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_flag_enum_has_fp32():
    from smd_amd import flags as F
    d = {f.name: f for f in F.ENGINE_FLAGS}["dtype"]
    assert tuple(d.choices) == ("bf16", "fp8", "fp32")


def test_netconfig_accepts_fp32_and_engine_names_the_three_precisions():
    from smd_amd.engine import DTYPES, FP32_REFUSAL, NetConfig
    assert NetConfig(dtype="fp32").dtype == "fp32" and DTYPES == ("bf16", "fp8", "fp32")
    assert "fp32 is an inference precision in this engine" in FP32_REFUSAL


def test_header_and_ctypes_table_agree_on_abi_8_and_the_fp32_entries():
    import smd_amd.lib as lib
    text = open(lib.HEADER_PATH).read()
    assert re.search(r"#define SMD_ABI_VERSION 8\b", text) and lib.ABI_VERSION == 8
    stable = set(lib.declared_symbols(lab=False))
    assert {"smd_gemm_f32", "smd_layernorm_f32", "smd_attention_f32", "smd_noise_embed_f32"} <= stable
    assert '"fp32" 0/1' in text


def test_train_cli_refuses_fp32_in_words_before_touching_the_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_ncsn.py"), "--synthetic", "--dtype=fp32"], capture_output=True,
                       text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0
    assert "fp32 is an inference precision in this engine" in r.stderr


def test_one_chain_under_fp32():
    import types
    import smd_amd.ncsn as N
    tr = types.SimpleNamespace(engine=types.SimpleNamespace(S=32, cfg=types.SimpleNamespace(mlp_dims=2048, dtype="fp32")))
    assert N.sampler_chain_sizes(tr, 256, True) == ([256], 0)
    tr.engine.cfg.dtype = "bf16"
    assert N.sampler_chain_sizes(tr, 256, True) == ([128, 128], 0)
