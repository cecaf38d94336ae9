"""What the GPU tests of the distillation kernels share (tests/test_gpu_distill_kernels.py, tests/test_gpu_distill_footprint.py):
the walk, the tables and the fp32 inputs of a distillation step, made once per case and never changed."""
import numpy as np
import torch

import _distill_ref as R

U = R.U
T, N = 16, 4
SHAPES = [(3, 32, 42), (2, 32, 8), (5, 1, 6), (2, 1, 8)]
KINDS = ("eps", "x0", "v")
BETAS = np.linspace(1e-3, 0.2, T).astype(np.float32)


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def ck(rc, what=""):
    import smd_amd.lib as lib
    lib.check(rc, what)


def bits(t):
    return t.detach().contiguous().view(torch.uint8).cpu()


def steps_for(B, bad=None):
    k = np.array([0, N - 1, 1, 1, 2], dtype=np.int32)[:B].copy()
    if bad is not None:
        k[min(1, B - 1)] = bad
    return k


_TABLES = {}


def tables(teacher, student, weighting="truncated_snr"):
    import smd_amd.schedule as S
    key = (teacher, student, weighting)
    if key not in _TABLES:
        tw, _ = S.distill_walk(T, N)
        _TABLES[key] = S.distill_tables(BETAS, tw, teacher, student, weighting)
    return _TABLES[key]


_CASES = {}


def case(B, S, C, teacher):
    """fp32 inputs of the three kernels for the in-range steps of ``steps_for(B)``, made once per (shape, teacher kind) and
    never changed: dict(x0, eps, z_t, out1, x1, z_m, out2, pred)"""
    import smd_amd.schedule as Sch
    key = (B, S, C, teacher)
    if key in _CASES:
        return _CASES[key]
    g = np.random.default_rng(27000 + B * 1000 + S * 10 + C)
    shape = (B, S, C)
    table, ref = tables(teacher, "x0")
    ap = Sch.alphas_cumprod(BETAS).astype(np.float64)
    tk = Sch.prediction_kind(teacher)
    k = steps_for(B)
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    x0 = f32(g.uniform(-0.8, 0.8, shape))
    eps = f32(g.standard_normal(shape))
    z_t = f32(R.noise(x0, eps, table, k)[0])
    lvl = lambda name: ap[ref[name][k]].reshape(B, 1, 1)
    out1 = f32(R.exact_output(tk, x0.astype(np.float64), z_t.astype(np.float64), lvl("t")) + 0.1 * g.standard_normal(shape))
    x1, z_m, _, _ = R.mid(z_t, out1, table, k)
    x1, z_m = f32(x1), f32(z_m)
    out2 = f32(R.exact_output(tk, x0.astype(np.float64), z_m.astype(np.float64), lvl("m")) + 0.1 * g.standard_normal(shape))
    pred = f32(g.standard_normal(shape))
    _CASES[key] = {n: torch.from_numpy(v) for n, v in dict(x0=x0, eps=eps, z_t=z_t, out1=out1, x1=x1, z_m=z_m, out2=out2,
                                                           pred=pred).items()}
    return _CASES[key]
