"""End-to-end parity, repeatability and data-parallel equivalence at the configurations bench.py times:
B = 256, C = 512, L6 H8 K2 (BASELINE config 2) and L8 H16 K3 (config 4), through the SHIPPED engine options
(side-stream weight gradients, 256x256 NT / TN GEMMs, paired / grouped wgrads, bf16 residual-gradient chain,
fused encoder kernels, hipGraph sampler).  At this size every kernel of the bench path is reached in situ
(8192-row GEMMs, 16-wave LayerNorms), unlike the B <= 6 cases of test_gpu_engine.py.

Reference functions: train_ncsn.py:260-288 (train_step), utils/losses.py:250-308 (diffusion_loss),
utils/ebm_utils.py:327-394 (sample_with_beta), models/ncsn.py:141-179.
Oracle: oracle/ddpm_oracle.py in fp32 on the host cores (fp64 at B = 256 costs minutes); tolerances are those
of SURVEY section 8c: rel-L2 <= 1e-2 on eps_hat and on the gradient, loss <= 5e-3 relative, Adam update <= 1e-4
of the update size (fp64 arithmetic on the engine's own gradient).
"""
import numpy as np
import pytest
import torch

import ddpm_oracle as O

pytestmark = pytest.mark.gpu
ORACLE_THREADS = 64          # the oracle runs at B = 256 here (tests/conftest.py)

BETAS = O.create_noise_schedule(1e-6, 0.01, 1000, "linear")
CONFIGS = {"base": dict(L=6, H=8, K=2), "large": dict(L=8, H=16, K=3)}
B = 256
C = 512


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def build(name, seed=0, dtype="bf16"):
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    kw = CONFIGS[name]
    ocfg = O.NetConfig(data_channels=C, num_layers=kw["L"], num_heads=kw["H"], num_mlp_layers=kw["K"])
    p = O.init_params(ocfg, seed, torch.float32)
    g = torch.Generator().manual_seed(seed + 1)
    for k in p:      # non-trivial biases / LayerNorm affine so that every epilogue term is exercised
        if k.endswith(".bias"):
            p[k] = 0.1 * torch.randn(p[k].shape, generator=g)
        elif k.endswith(".scale"):
            p[k] = 1 + 0.1 * torch.randn(p[k].shape, generator=g)
    cfg = NetConfig(architecture="TransformerDDPM", data_channels=C, seq_len=32, num_layers=kw["L"], num_heads=kw["H"],
                    num_mlp_layers=kw["K"], num_timesteps=1000, dtype=dtype)
    model = N.Model(cfg, "cuda:0", seed=None)
    model.engine.load_named(p)
    return ocfg, p, model


def draws(seed=1234):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.clamp(0.25 * torch.randn(B, 32, C, generator=g), -1, 1)
    labels = torch.randint(1, 1001, (B,), generator=g)
    labels[0] = 1                                     # the alpha = 1 corner of the jax-0.2.8 uniform quirk
    eps = torch.randn(B, 32, C, generator=g)
    return x0, labels, eps, g


@pytest.mark.parametrize("name", ["base", "large"])
def test_train_step_parity_at_bench_size(name):
    ocfg, p, model = build(name)
    x0, labels, eps, _ = draws()
    leaf = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    base_model = O.make_model(leaf, ocfg)
    seen = {}

    def capturing(x, cond):
        out = base_model(x, cond)
        seen["pred"] = out.detach()
        return out

    loss_ref = O.diffusion_loss(x0, capturing, BETAS, labels.numpy(), eps, "none")
    loss_ref.mean().backward()

    eng = model.train_engine(ema=True)                # default options: side stream on, nt256 / tn256, fused encoder
    eng.set_schedule(BETAS, with_sampler=False)
    eng.bind(B, training=True)
    before = eng.params.clone()
    eng.loss_backward(x0.cuda(), labels.int().cuda(), eps.cuda(), stage=0)
    torch.cuda.synchronize()
    e_pred = rel(eng.last_pred(), seen["pred"])
    e_loss = rel(eng.loss_per_sample(), loss_ref)
    m_eng, m_ref = float(eng.loss_per_sample().mean()), float(loss_ref.mean())
    print(f"[{name}] eps_hat rel {e_pred:.3e}; per-sample loss rel {e_loss:.3e}; mean loss {m_eng:.6f} vs {m_ref:.6f}")
    assert e_pred < 1e-2
    assert abs(m_eng - m_ref) / m_ref < 5e-3
    assert e_loss < 1e-2
    gv = eng.named_views(eng.grads)
    worst, worst_name, num, den = 0.0, "", 0.0, 0.0
    for k, v in leaf.items():
        r = rel(gv[k], v.grad)
        if r > worst:
            worst, worst_name = r, k
        num += float((gv[k].double().cpu() - v.grad.double()).pow(2).sum())
        den += float(v.grad.double().pow(2).sum())
    total = (num / den) ** 0.5
    print(f"[{name}] gradient whole-vector rel {total:.3e}; worst tensor {worst_name} {worst:.3e}")
    assert total < 1e-2
    assert worst < 6e-2

    # one optimiser update on the engine's own gradient: clip + Adam + EMA in fp64 (train_ncsn.py:284-287)
    grads = {k: v.double().cpu().clone() for k, v in gv.items()}
    cur = {k: v.double() for k, v in p.items()}
    clipped, norm_after = O.clip_grads(grads, 1.0)
    st = O.AdamState()
    new = O.adam_update(cur, clipped, st, 1e-3)
    ema = O.ema_update(cur, new, 0.999)
    eng.optimizer_step(1e-3, 1.0, 1, 1.0, 0.999)
    torch.cuda.synchronize()
    pv, ev = eng.named_views(eng.params), eng.named_views(eng.ema)
    num = sum(float((pv[k].double().cpu() - new[k]).pow(2).sum()) for k in new)
    den = sum(float((new[k] - cur[k]).pow(2).sum()) for k in new)
    m = eng.metrics.cpu()
    print(f"[{name}] Adam update rel err {(num / den) ** 0.5:.3e}; |g| {float(m[0]):.4f} -> {float(m[1]):.4f}")
    assert (num / den) ** 0.5 < 1e-4
    assert abs(float(m[1]) - float(norm_after)) / float(norm_after) < 1e-5
    assert max(rel(ev[k], ema[k]) for k in ema) < 1e-6
    assert not torch.equal(before, eng.params)


@pytest.mark.parametrize("name,dtype", [("base", "bf16"), ("large", "bf16"), ("base", "fp8"), ("large", "fp8")])
def test_reverse_steps_through_the_captured_graph(name, dtype):
    """Three reverse iterations t = 999, 998, 997 with explicit z draws, replayed from ONE captured hipGraph (the
    path bench.py and sample_ncsn.py time), against the oracle rollout (utils/ebm_utils.py:327-394).  fp8: the e4m3
    DenseResBlock GEMMs inside the captured step (`extra_configs.base_fp8 / large_fp8` of the bench line); the state
    tolerance stays 1e-2, the eps_hat-norm metric gets the fp8 forward tolerance of SURVEY 8c (5e-2)."""
    import smd_amd.lib as lib
    ocfg, p, model = build(name, dtype=dtype)
    g = torch.Generator().manual_seed(4321)
    init = torch.randn(B, 32, C, generator=g)
    zs = {t: torch.randn(B, 32, C, generator=g) for t in (999, 998, 997)}
    with torch.no_grad():
        ref, _, mref = O.diffusion_dynamics(O.make_model(p, ocfg), BETAS, init, lambda t: zs[t], t_stop=997)
    eng = model.engine
    eng.set_schedule(BETAS, with_sampler=True)
    eng.bind(B, training=False)
    eng.prepare_sampler()
    dev = eng.device
    x = init.to(dev).clone()
    zbuf = zs[999].to(dev).clone()
    t_ptr = torch.tensor([999], dtype=torch.int32, device=dev)
    metrics_partial = torch.zeros(1000, B, 3, device=dev)
    collection = torch.zeros(41, B, 32, C, device=dev)
    io = lib.SampleIO()
    io.x, io.t_ptr, io.z_in = x.data_ptr(), t_ptr.data_ptr(), zbuf.data_ptr()
    io.metrics_partial, io.collection, io.slot_table = metrics_partial.data_ptr(), collection.data_ptr(), eng.slot_table.data_ptr()
    eng.load_state(x)
    # warm-up on a side stream (allocations, lazy module loads), then restore the state and capture one step
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        eng.sample_step(io)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    x.copy_(init.to(dev)); t_ptr.fill_(999); metrics_partial.zero_(); collection.zero_()
    eng.load_state(x)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.sample_step(io)
    x.copy_(init.to(dev)); t_ptr.fill_(999); metrics_partial.zero_()
    eng.load_state(x)
    for t in (999, 998, 997):
        zbuf.copy_(zs[t].to(dev))
        graph.replay()
    torch.cuda.synchronize()
    assert int(t_ptr.item()) == 996
    e = rel(x, ref)
    per_t = (metrics_partial.sum(dim=1) / float(B * C)).cpu()           # rows indexed by t: (grad, step, noise)
    got = torch.stack([per_t[[999, 998, 997], 0], per_t[[999, 998, 997], 1], per_t[[999, 998, 997], 2]])
    want = torch.stack([mref[0, :3, 0], mref[1, :3, 0], mref[3, :3, 0]])
    print(f"[{name} {dtype}] 3 graph-replayed reverse steps: state rel {e:.3e}; metrics rel {rel(got, want):.3e}")
    assert e < 1e-2
    assert rel(got, want) < (1e-2 if dtype == "bf16" else 5e-2)


@pytest.mark.parametrize("name,dtype,repeats", [("base", "bf16", 500), ("large", "bf16", 100), ("base", "fp8", 100)])
def test_train_step_bitwise_repeatable(name, dtype, repeats):
    """same inputs twice => bitwise equal, for the whole training step with the shipped defaults
    (two HIP streams inside the engine).  `repeats` x loss_backward on identical inputs (500 at the headline configuration:
    the event this gates -- a LayerNorm backward disturbed by a co-resident weight-gradient workgroup, DESIGN section 6 --
    showed up in 1-2 % of the steps of the worst default build), then two identical optimiser trajectories from the same
    state.  Every configuration the bench line times is covered: base, large, and the e4m3 path."""
    _, p, model = build(name, dtype=dtype)
    x0, labels, eps, _ = draws()
    eng = model.train_engine(ema=False)
    eng.set_schedule(BETAS, with_sampler=False)
    eng.bind(B, training=True)
    xd, ld, ed = x0.cuda(), labels.int().cuda(), eps.cuda()
    ref_g = ref_l = ref_p = None
    bad = []
    for it in range(repeats):
        eng.loss_backward(xd, ld, ed, stage=0)
        torch.cuda.synchronize()
        if ref_g is None:
            ref_g, ref_l, ref_p = eng.grads.clone(), eng.loss_per_sample().clone(), eng.last_pred().clone()
            continue
        if not (torch.equal(eng.grads, ref_g) and torch.equal(eng.loss_per_sample(), ref_l) and torch.equal(eng.last_pred(), ref_p)):
            gv, rv = eng.named_views(eng.grads), eng.named_views(ref_g)
            bad.append((it, [k for k in gv if not torch.equal(gv[k], rv[k])][:4]))
    assert not bad, f"loss_backward is not bitwise repeatable: {len(bad)} of {repeats - 1} repeats differ, first {bad[:3]}"

    def trajectory():
        eng.params.copy_(start)
        eng.m.zero_(); eng.v.zero_(); eng.step_counter.zero_()
        eng.refresh_weights()
        for _ in range(4):
            eng.loss_backward(xd, None, None, seed=11, stage=0)      # in-kernel Philox draws, keyed by the step counter
            eng.optimizer_step(1e-3, 0.98, 10000, 1.0, 0.999)
        torch.cuda.synchronize()
        return eng.params.clone()

    start = eng.params.clone()
    a = trajectory()
    b = trajectory()
    assert torch.equal(a, b), "two identical 4-step training trajectories differ"


def test_data_parallel_engine_equivalence_single_gpu():
    """SURVEY section 4 "Distributed": N ranks' staged backward (stage 1 = loss + forward + output-stage backward,
    the point where trainer.py starts the first all-reduce; stage 2 = encoder backward) on their batch shards,
    SUMmed, equals the 1-rank step on the concatenated batch -- including the 1/(global_batch*S*C) loss scaling and
    the Philox label / eps draws keyed by the global sample index (sample_offset).  Two ranks are emulated on one GPU
    by running the shards one after the other on a second engine with the same parameters."""
    import smd_amd.ncsn as N
    _, p, joint = build("base")
    shard = N.Model(joint.cfg, "cuda:0", seed=None, share_params_with=joint)
    x0, _, _, _ = draws()
    xd = x0.cuda()
    ej = joint.train_engine(ema=False)
    ej.set_schedule(BETAS, with_sampler=False)
    ej.bind(B, training=True)
    ej.loss_backward(xd, None, None, seed=5, sample_offset=0, global_batch=B, stage=0)
    torch.cuda.synchronize()
    g_joint, l_joint = ej.grads.clone(), ej.loss_per_sample().clone()

    es = shard.train_engine(ema=False)
    es.set_schedule(BETAS, with_sampler=False)
    half = B // 2
    es.bind(half, training=True)
    total = torch.zeros_like(g_joint)
    for r in range(2):
        xs = xd[r * half:(r + 1) * half].contiguous()
        es.loss_backward(xs, None, None, seed=5, sample_offset=r * half, global_batch=B, stage=1)
        torch.cuda.synchronize()
        head = es.grads[es.head_offset:].clone()          # what the first all-reduce bucket would carry
        es.loss_backward(None, None, None, seed=5, sample_offset=r * half, global_batch=B, stage=2)
        torch.cuda.synchronize()
        assert torch.equal(es.grads[es.head_offset:], head), "stage 2 touched output-stage gradients after their all-reduce started"
        total += es.grads
        e_l = rel(es.loss_per_sample(), l_joint[r * half:(r + 1) * half])
        print(f"rank {r}: per-sample loss vs the joint run rel {e_l:.3e}")
        assert e_l < 1e-6                                   # identical Philox draws (labels, eps) and forward
    gj, gt = ej.named_views(g_joint), ej.named_views(total)
    errs = sorted(((rel(gt[k], gj[k]), k) for k in gj), reverse=True)
    worst, worst_name = errs[0]
    whole = rel(total, g_joint)
    print(f"sum of 2 shard gradients vs joint: whole-vector rel {whole:.3e}, worst tensor {worst_name} {worst:.3e} "
          f"(|g| {float(gj[worst_name].norm()):.3e})")
    # Every bf16 rounding on the way is per row, so the shards see bitwise the same activations (the per-sample losses
    # above are bitwise equal); what differs is the fp32 summation order of the row contractions (4096 + 4096 rows with
    # a different split-K partition vs 8192), amplified by cancellation in the small bias / LayerNorm tensors.
    # Measured: 4.8e-5 whole vector, 1.8e-3 worst tensor.
    assert whole < 2e-4
    assert worst < 1e-2


def test_stem_gradient_bucket_events_gate_exactly_their_layer():
    """Data-parallel early start (engine option dp_layer_events, trainer.GradComm(layer_buckets=True)): the stem backward records
    one event per encoder layer as soon as that layer's gradients are final.  A second stream that waits ONLY for bucket b's
    event must read the final gradient of that layer -- from a NaN-poisoned buffer, while the layers below are still running."""
    _, p, model = build("base")
    x0, labels, eps, _ = draws()
    eng = model.train_engine(ema=False)
    eng.set_schedule(BETAS, with_sampler=False)
    eng.bind(B, training=True)
    eng.set_option("dp_layer_events", 1)
    buckets = eng.grad_buckets()
    assert len(buckets) == 6 and buckets[-1][0] == 0 and buckets[0][0] + buckets[0][1] == eng.head_offset
    assert all(buckets[i + 1][0] + buckets[i + 1][1] == buckets[i][0] for i in range(5))       # backward order, no gaps
    xd, ld, ed = x0.cuda(), labels.int().cuda(), eps.cuda()
    comm = torch.cuda.Stream()
    g = eng.grads
    for rep in range(3):
        g.fill_(float("nan"))
        eng.loss_backward(xd, ld, ed, stage=1)
        eng.loss_backward(None, None, None, stage=2)
        snaps = []
        for b, (off, ln) in enumerate(buckets[:-1]):
            eng.wait_grad_bucket(b, comm)
            with torch.cuda.stream(comm):
                snaps.append(g[off:off + ln].clone())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g).all())
        for (off, ln), snap in zip(buckets[:-1], snaps):
            assert torch.equal(snap, g[off:off + ln]), "a bucket event fired before its layer's gradients were final"
    eng.set_option("dp_layer_events", 0)
    ref = g.clone()
    eng.loss_backward(xd, ld, ed, stage=0)
    torch.cuda.synchronize()
    assert torch.equal(eng.grads, ref)                     # the per-layer LayerNorm reductions change nothing in the result


@pytest.mark.parametrize("arch,C,B", [("TransformerDDPM", 512, 256), ("TransformerDDPM", 42, 8), ("DenseDDPM", 512, 64),
                                      ("DenseDDPM", 42, 64)])
def test_every_gradient_element_is_written_without_the_memset(arch, C, B):
    """The default path no longer zeroes the 102 MB gradient buffer before a step (engine option grad_memset = 2): every
    element must be overwritten.  Poison the buffer with NaN, run a step -- also in the two data-parallel stages -- and
    require the result to be finite and bitwise equal to the same step with the memset forced."""
    import smd_amd.ncsn as N
    from smd_amd.engine import NetConfig
    cfg = NetConfig(architecture=arch, data_channels=C, seq_len=32, num_timesteps=1000)
    model = N.Model(cfg, "cuda:0", seed=3)
    eng = model.train_engine(ema=False)
    eng.set_schedule(BETAS, with_sampler=False)
    eng.bind(B, training=True)
    g = torch.Generator().manual_seed(9)
    shape = (B, C) if arch == "DenseDDPM" else (B, 32, C)
    x0 = torch.clamp(0.25 * torch.randn(*shape, generator=g), -1, 1).cuda()
    labels = torch.randint(1, 1001, (B,), generator=g).int().cuda()
    eps = torch.randn(*shape, generator=g).cuda()
    eng.set_option("grad_memset", 1)
    eng.loss_backward(x0, labels, eps, stage=0)
    torch.cuda.synchronize()
    ref = eng.grads.clone()
    assert torch.isfinite(ref).all()
    eng.set_option("grad_memset", 2)
    for stages in ((0,), (1, 2)):
        eng.grads.fill_(float("nan"))
        for st_ in stages:
            eng.loss_backward(x0 if st_ != 2 else None, labels if st_ != 2 else None, eps if st_ != 2 else None, stage=st_)
        torch.cuda.synchronize()
        bad = int((~torch.isfinite(eng.grads)).sum())
        assert bad == 0, f"{bad} gradient elements were not written (stages {stages})"
        assert torch.equal(eng.grads, ref)


def test_bench_script_with_two_ranks_on_one_gpu():
    """bench.py's multi-rank path end to end on a one-GPU box: `--gpus 2` launches its own two ranks, which share cuda:0 over
    gloo (test hook SMD_BENCH_SHARE_DEVICE): sharded synthetic inputs, the two-stage gradient all-reduce of trainer.GradComm
    between the two loss_backward stages, barriers, MAX over ranks, one JSON line from rank 0 with n_gpus = 2.  The numbers
    are not measurements (two ranks time-slice one GPU, the collective goes through the host) and the line says so."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMD_BENCH_SHARE_DEVICE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--repeats", "1",
                        "--no-roofline-microbench"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                   # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 512
    assert "TEST RUN" in d["data"]
    assert d["value"] > 0 and np.isfinite(d["final_loss"]) and 0.5 < d["final_loss"] < 3.0
    assert d["extra_configs"] is None and d["cpu_baseline"] is None          # single-GPU extras stay out of a multi-rank line
    # the line proves what ran between the ranks: library, world size, shape of the exchange, measured exposed communication
    dp = d["config"]["dp"]
    assert dp["backend"] == "gloo" and dp["world_size"] == 2 and dp["algorithm"] == "all_reduce" and dp["layer_buckets"] is False
    assert dp["collectives_per_step"] == 2.0                                 # output-stage slice + stem slice, nothing else
    assert dp["exposed_comm_us"] is not None and dp["exposed_comm_us"] >= 0
    # ... and on which devices: one identity per rank (GPU UUID and / or PCI address), here twice the same one -- which the script
    # accepts only because of the test hook (without it, ranks that share a device print no line: tests/test_host.py)
    assert len(dp["devices"]) == 2 and dp["devices"][0] == dp["devices"][1] and dp["distinct_devices"] == 1
    assert d["config"]["devices"] == dp["devices"] and any(t in dp["devices"][0] for t in ("uuid:", "pci:", "ordinal:"))


def test_bench_plain_run_times_its_steps_and_dumps_repeatable_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one timed block of exactly K steps, none of the --full legs, and
    the outputs of the last timed step on disk.  Two runs with the same arguments write bitwise the same arrays (same inputs, the
    training step and the pipelined walk are bitwise repeatable)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SMD_BENCH_SHARE_DEVICE"):
        env.pop(k, None)
    outs = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 4 and d["repeats"] == 1 and len(d["block_values"]) == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3          # value and ms_per_step describe one block
        assert d["cpu_baseline"] is None and d["extra_configs"] is None and d["sampler_walk"] is None
        assert d["roofline"]["achieved"] is None
        outs.append({n: np.load(tmp_path / run / f"{n}.npy")
                     for n in ("train_loss_per_sample", "train_metrics", "params_sample", "sample_x")})
    a, b = outs
    assert a["train_loss_per_sample"].shape == (256,) and a["sample_x"].shape == (256, 32, 512)
    assert a["params_sample"].shape == (1 << 22,) and a["params_sample"].dtype == np.float32 and a["train_metrics"].dtype == np.float64
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert abs(a["train_metrics"][0] - a["train_loss_per_sample"].mean()) < 1e-5 * a["train_metrics"][0]
    for n in a:
        assert np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n


def test_bench_dp_dry_run_on_one_gpu():
    """`bench.py --dp-dry-run`: the multi-GPU train step on CUDA gradient tensors with a communication stream that runs kernels of a
    collective's shape beside the backward pass (two ranks on cuda:0 over gloo).  The reduced gradient and the parameters after 3
    steps must be bitwise the same with that load, with it again, and without it, and equal on both ranks."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SMD_BENCH_SHARE_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--dp-dry-run", "--steps", "3", "--warmup", "1", "--dp-layer-buckets", "1"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])["dp_dry_run"]
    assert d["ok"] and d["ranks_agree"] and all(d["bitwise"].values()), d
    assert d["comm"]["emulated_load"] in (True, False) and d["comm"]["layer_buckets"] is True and d["world"] == 2
