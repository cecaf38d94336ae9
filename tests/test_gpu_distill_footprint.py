"""Footprint of the three distillation kernels with tests/_footprint.py: only the outputs are written --
the inputs, the table and the steps come back bit for bit, the red zones around every output hold their sentinel -- and the
rows of a no-op sample keep the canary they started with, under both sentinel patterns.  The outputs are contiguous (no
padding columns), so the red zones and the no-op rows are all there is besides the outputs.  Shapes: one vector and one
scalar form, (2, 32, 8) and (5, 1, 6)."""
import numpy as np
import pytest
import torch

import _footprint as F
from _distill_cases import N, case, ck, st, steps_for, tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import smd_amd.lib as lib
    return lib.get_lib()


def _rows_hold(t, rows, fill):
    want = torch.tensor([fill & 0xFF, fill >> 8], dtype=torch.uint8).repeat(2)
    return bool((t[rows].contiguous().view(torch.uint8).reshape(-1, 4).cpu() == want).all())


@pytest.mark.parametrize("fill", F.PATTERNS)
@pytest.mark.parametrize("B,S,C", [(2, 32, 8), (5, 1, 6)])
def test_only_the_outputs_are_written(L, dev, B, S, C, fill):
    table, _ = tables("v", "v")
    c = {n: v.to(dev) for n, v in case(B, S, C, "v").items()}
    k = steps_for(B, bad=N + 3)
    dead = [i for i, v in enumerate(k) if not 0 <= v < N]
    live = [i for i in range(B) if i not in dead]
    table_h = F.guarded_like(torch.from_numpy(table), dev, fill=fill)[1]
    k_h = F.guarded_like(torch.from_numpy(k), dev, fill=fill)[1]
    ins = {n: F.guarded_like(v.cpu(), dev, fill=fill)[1] for n, v in c.items()}
    g = lambda shape: F.guarded(shape, torch.float32, dev, fill=fill)
    full, per = (B, S, C), (B,)

    def check(outs):
        torch.cuda.synchronize()
        for name, (view, h) in outs.items():
            h.assert_untouched(name)
            assert _rows_hold(view, dead, fill), f"{name}: the rows of the no-op sample changed"
            assert torch.isfinite(view[live]).all(), f"{name}: the live rows were written"

    outs = dict(z_t=g(full), level=g(per), eps=g(full))
    with F.unchanged(table_h, k_h, ins["x0"]):
        ck(L.smd_distill_noise(ins["x0"].ptr, B, S, C, table_h.ptr, N, k_h.ptr, outs["eps"][1].ptr, 1, 3, 4, 0, 9, None,
                               outs["z_t"][1].ptr, outs["level"][1].ptr, st()), "distill_noise")
        check(outs)
    outs = dict(x1=g(full), z_m=g(full), level=g(per))
    with F.unchanged(table_h, k_h, ins["z_t"], ins["out1"]):
        ck(L.smd_distill_mid(ins["z_t"].ptr, ins["out1"].ptr, B, S, C, table_h.ptr, N, k_h.ptr, outs["x1"][1].ptr, outs["z_m"][1].ptr,
                             outs["level"][1].ptr, st()), "distill_mid")
        check(outs)
    for kind in (0, 1, 2):
        outs = dict(loss=g(per), weight=g(per), dpred=g(full), target=g(full))
        with F.unchanged(table_h, k_h, *[ins[n] for n in ("x1", "z_m", "out2", "z_t", "pred")]):
            ck(L.smd_distill_loss(ins["x1"].ptr, ins["z_m"].ptr, ins["out2"].ptr, ins["z_t"].ptr, ins["pred"].ptr, kind, B, S, C,
                                  table_h.ptr, N, k_h.ptr, None, float(np.float32(1.0 / (B * S * C))), outs["loss"][1].ptr,
                                  outs["weight"][1].ptr, outs["dpred"][1].ptr, outs["target"][1].ptr, st()), "distill_loss")
            check(outs)
