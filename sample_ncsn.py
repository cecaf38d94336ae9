"""Drop-in for the reference's ``python sample_ncsn.py --flagfile=... --sample_seed --sample_size
--sampling_dir`` on the MI355X HIP engine: unconditional generation, infilling (--infill) and
interpolation (--interpolate) for DDPM checkpoints, writing {sampling_dir}/ncsn/{generated,
collection,real}.pkl in the reference's layout (sample_ncsn.py:368-471).  --ddim_steps=K walks K of the
schedule's timesteps with the strided (DDIM) sampler instead of all of them, in all three modes.  --ddim_order=2
--ddim_spacing=logsnr makes that walk the second-order multistep solver DPM-Solver++(2M) on a lambda-uniform grid, --ddim_solver=adams3 /
adams3_pc a third-order exponential Adams solver on it.  --compute_bound
evaluates the per-timestep variational bound on the eval examples first (--bound_only: and stops there).

Multi-GPU sampling is embarrassingly parallel: under torch.distributed.run each rank generates a
contiguous shard of the samples (Philox counters are keyed by the GLOBAL sample index, so the
result does not depend on the number of GPUs) and rank 0 gathers and writes the files.
"""
from __future__ import annotations

import logging
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import smd_amd  # noqa: E402,F401
from smd_amd import flags as F  # noqa: E402
from smd_amd import schedule  # noqa: E402

log = logging.getLogger("smd_amd")


def load_model(FLAGS, shape, device):
    """sample_ncsn.py:331-342: dummy-parameter model + restore_checkpoint.  The reference samples
    from optimizer.target (raw weights) even when an EMA was trained (:353-354); --sample_ema opts
    into the EMA weights."""
    from smd_amd import checkpoint, ncsn
    model_kwargs = dict(num_layers=FLAGS.num_layers, num_heads=FLAGS.num_heads,
                        num_mlp_layers=FLAGS.num_mlp_layers, mlp_dims=FLAGS.mlp_dims)
    rng = ncsn.make_key(FLAGS.sample_seed, FLAGS.rng_impl)
    rng, model_rng = ncsn.split(rng)
    model = ncsn.create_model(model_rng, shape, model_kwargs, batch_size=1, verbose=True,
                              architecture=FLAGS.architecture, num_timesteps=FLAGS.num_sigmas, device=device, dtype=FLAGS.dtype,
                              init=False)                       # the weights come from the checkpoint (sample_ncsn.py:331-342)
    found = (checkpoint.load_ema_params if FLAGS.sample_ema else
             lambda d, e: checkpoint.restore_checkpoint(d, e, load_optimizer_state=False)[0])(FLAGS.model_dir, model.engine)
    if not found:
        log.warning("no checkpoint under %s: sampling from freshly initialised weights", FLAGS.model_dir)
        ncsn.init_model(model, model_rng)
    return model, rng


def _prediction(FLAGS) -> str:
    """The resolved --prediction (main settles it against the checkpoint before anything runs); eps when it was never given."""
    return getattr(FLAGS, "prediction", "") or "eps"


def resolve_prediction_flag(FLAGS) -> str:
    """--prediction against what the checkpoint under --model_dir records (smd_amd.checkpoint.resolve_prediction): empty takes
    the checkpoint's kind (eps when it names none: a flax-format file, an older checkpoint, no checkpoint), a contradiction is a
    ValueError.  A kind other than eps needs --sampling=ddpm."""
    from smd_amd import checkpoint
    kind = checkpoint.resolve_prediction(FLAGS.prediction, checkpoint.checkpoint_prediction(FLAGS.model_dir),
                                         f"the checkpoint under {FLAGS.model_dir}")
    if kind != "eps" and FLAGS.sampling != "ddpm":
        raise ValueError(f"--prediction={kind} needs --sampling=ddpm (got --sampling={FLAGS.sampling}): the Langevin samplers "
                         "(--sampling=ald, --sampling=cas) take the network's output as a score")
    return kind


def resolve_distill_walk(FLAGS):
    """The walk a distilled student's checkpoint records (``distill_timesteps``), or None.  With
    --sampling=ddpm such a checkpoint is sampled on that walk by the strided sampler: --ddim_steps unset takes its length, another
    number is refused, --ddim_order / --ddim_eta / --infill / --interpolate go through the same walk.  Before the GPU is touched."""
    from smd_amd import checkpoint
    walk = checkpoint.checkpoint_distill_walk(FLAGS.model_dir) if FLAGS.sampling == "ddpm" else None
    if walk is None:
        return None
    where = f"the checkpoint under {FLAGS.model_dir} was distilled to the {len(walk)} timesteps {checkpoint.format_walk(walk)}"
    if FLAGS.ddim_steps and FLAGS.ddim_steps != len(walk):
        raise SystemExit(f"--ddim_steps={FLAGS.ddim_steps}: {where}; drop the flag or pass --ddim_steps={len(walk)}")
    if FLAGS.ddim_spacing != "uniform":
        raise SystemExit(f"--ddim_spacing={FLAGS.ddim_spacing} chooses the timesteps itself: {where}")
    if FLAGS.ddim_encode:
        raise SystemExit(f"--ddim_encode inverts an evenly spaced walk: {where}")
    if max(walk) >= FLAGS.num_sigmas:
        raise SystemExit(f"--num_sigmas={FLAGS.num_sigmas}: {where}")
    FLAGS.ddim_steps = len(walk)
    return walk


def generate_samples(FLAGS, model, rng, sample_shape, num_samples, sigmas, sample_offset=0, global_num_samples=None, walk=None,
                     analytic=None):
    """sample_ncsn.py:313-365."""
    from smd_amd import ncsn
    rng, sample_rng = ncsn.split(rng)
    t0 = time.time()
    generated, collection, ld_metrics = ncsn.sample(
        model, sigmas, sample_rng, sample_shape, num_samples=num_samples, sampling=FLAGS.sampling,
        epsilon=FLAGS.ld_epsilon, steps=FLAGS.ld_steps, denoise=FLAGS.denoise, sample_offset=sample_offset,
        use_graph=FLAGS.graph, global_num_samples=global_num_samples, ddim_steps=FLAGS.ddim_steps, ddim_eta=FLAGS.ddim_eta,
        ddim_order=FLAGS.ddim_order, ddim_spacing=FLAGS.ddim_spacing, prediction=_prediction(FLAGS), ddim_timesteps=walk,
        analytic=analytic, ddim_solver=FLAGS.ddim_solver)
    torch.cuda.synchronize()
    log.info("Generated samples in %f seconds", time.time() - t0)
    return generated, collection, ld_metrics


def infill_samples(FLAGS, model, rng, samples, masks, sigmas, sample_offset=0, global_num_samples=None, walk=None, analytic=None):
    """sample_ncsn.py:189-242 (init ~ U[0,1) like :228: jax.random.uniform with --rng_impl=threefry, torch's device
    generator otherwise)."""
    from smd_amd import jax_random, ncsn
    init_rng, ld_rng = ncsn.split(rng)
    if isinstance(init_rng, jax_random.ThreefryKey):
        per = int(np.prod(samples.shape[1:]))
        n_glob = (global_num_samples or (len(samples) + sample_offset)) * per
        init = jax_random.uniform(init_rng, samples.shape, model.engine.device, n_total=n_glob, offset=sample_offset * per)
    else:
        g = torch.Generator(device=model.engine.device).manual_seed(init_rng.seed & 0x7FFFFFFFFFFFFFFF)
        init = torch.rand(samples.shape, generator=g, device=model.engine.device)
    if FLAGS.sampling == "ald":                                             # :219-221
        generated, collection, ld_metrics = ncsn.annealed_langevin_dynamics(
            ld_rng, model, sigmas, init, FLAGS.ld_epsilon, FLAGS.ld_steps, FLAGS.denoise, True,
            infill_samples=samples, infill_masks=masks, sample_offset=sample_offset, global_num_samples=global_num_samples)
        return generated, collection, ncsn.collate_sampling_metrics(ld_metrics.cpu().numpy())
    if FLAGS.sampling == "cas":                                             # :222-223 -> NotImplementedError (:228-229)
        ncsn.consistent_langevin_dynamics(ld_rng, model, sigmas, init, FLAGS.ld_epsilon, FLAGS.ld_steps, FLAGS.denoise, True)
    if FLAGS.ddim_steps:
        generated, collection, ld_metrics = ncsn.strided_dynamics(
            ld_rng, model, sigmas, init, FLAGS.ddim_steps, FLAGS.ddim_eta, True, infill_samples=samples, infill_masks=masks,
            use_graph=FLAGS.graph, sample_offset=sample_offset, global_num_samples=global_num_samples, order=FLAGS.ddim_order,
            spacing=FLAGS.ddim_spacing, prediction=_prediction(FLAGS), timesteps=walk, analytic=analytic,
            solver=FLAGS.ddim_solver)
        return generated, collection, ncsn.collate_sampling_metrics(ld_metrics.cpu().numpy())
    generated, collection, ld_metrics = ncsn.diffusion_dynamics(
        ld_rng, model, sigmas, init, FLAGS.ld_epsilon, FLAGS.ld_steps, FLAGS.denoise, True,
        infill_samples=samples, infill_masks=masks, use_graph=FLAGS.graph, sample_offset=sample_offset,
        global_num_samples=global_num_samples, prediction=_prediction(FLAGS))
    return generated, collection, ncsn.collate_sampling_metrics(ld_metrics.cpu().numpy())


def diffusion_stochastic_encoder(samples, sigmas, rng, device="cuda:0", sample_offset=0, global_num_samples=None):
    """sample_ncsn.py:245-266: z = sqrt(ap[T]) x + sqrt(1-ap[T]) noise.  alphas_prod[T] is one past
    the end upstream; JAX clamps the gather, i.e. it uses ap[T-1] (SURVEY quirks ledger).  ``rng`` is the first
    child of split(PRNGKey(seed)) -- the reference draws the noise from it, not from noise_rng (:262-263)."""
    from smd_amd import jax_random
    ap = schedule.alphas_cumprod(sigmas)
    a_T = float(ap[-1])
    if isinstance(rng, jax_random.ThreefryKey):
        per = int(np.prod(samples.shape[1:]))
        n_glob = (global_num_samples or (len(samples) + sample_offset)) * per
        noise = jax_random.normal(rng, samples.shape, device, n_total=n_glob, offset=sample_offset * per).cpu().numpy()
    else:
        g = torch.Generator().manual_seed(rng.seed & 0x7FFFFFFFFFFFFFFF)
        noise = torch.randn(samples.shape, generator=g).numpy()
    return np.sqrt(a_T) * samples + np.sqrt(1 - a_T) * noise


def interpolate_samples(model, sigmas, real, lo, hi, rng, sample_seed, rng_impl, dev, use_graph=True, points=9, ddim_steps=0,
                        ddim_eta=0.0, ddim_encode=False, ddim_order=1, ddim_spacing="uniform", prediction="eps", walk=None,
                        analytic=None, ddim_solver="default"):
    """sample_ncsn.py:425-435 + diffusion_decoder (:269-310) for this rank's rows [lo, hi): goals = roll(starts, 1); both are
    encoded with the same key (the same noise); every one of the 9 interpolated latents is decoded with the SAME
    ld_rng = split(PRNGKey(sample_seed), 3)[1].  Returns (generated (9, n, ...), collection (9, 41, n, ...), collated metrics).
    ``ddim_steps`` > 0: the points are decoded with the strided sampler; with ``ddim_encode`` starts and goals are encoded by its
    deterministic inversion (ncsn.ddim_encode) instead of the single re-noising.  ``ddim_order`` / ``ddim_spacing``: the solver
    and the grid of the decoding walks (ncsn.strided_dynamics), ``ddim_solver`` its ``solver``; ``prediction``: what the network's output means, for the
    inversion and every decoding walk."""
    from smd_amd import ncsn
    num = len(real)
    starts = real[lo:hi]
    goals = np.roll(real, shift=1, axis=0)[lo:hi]
    if ddim_steps and ddim_encode:
        zs, zg = (ncsn.ddim_encode(model, sigmas, np.ascontiguousarray(v, dtype=np.float32), ddim_steps, use_graph=use_graph,
                                   prediction=prediction).cpu().numpy()
                  for v in (starts, goals))
    else:
        zs, zg = (diffusion_stochastic_encoder(v, sigmas, rng, dev, lo, num) for v in (starts, goals))
    _, ld_rng, _ = ncsn.split(ncsn.make_key(sample_seed, rng_impl), num=3)                 # :271-272 (the root key)
    gens, colls = [], []
    for i, alpha in enumerate(np.linspace(0.0, 1.0, points)):
        z = ((1 - alpha) * zs + alpha * zg).astype(np.float32)
        if ddim_steps:
            g, c, ld = ncsn.strided_dynamics(ld_rng, model, sigmas, z, ddim_steps, ddim_eta, use_graph=use_graph, sample_offset=lo,
                                             global_num_samples=num, order=ddim_order, spacing=ddim_spacing, prediction=prediction,
                                             timesteps=walk, analytic=analytic, solver=ddim_solver)
        else:
            g, c, ld = ncsn.diffusion_dynamics(ld_rng, model, sigmas, z, use_graph=use_graph, sample_offset=lo, global_num_samples=num,
                                               prediction=prediction)
        gens.append(g.cpu().numpy())
        colls.append(c.cpu().numpy())
        log.info("Generated samples %i out of %i", i, points)
    return np.stack(gens), np.stack(colls), ncsn.collate_sampling_metrics(ld.cpu().numpy())


NN_METRICS = ("improved_precision", "improved_recall", "improved_f1", "ipr_realism")      # --nn_metrics computes these
METRICS_KMEANS = ("precision", "recall", "f1", "ndb")                                    # PRD histogram and NDB: not computed
METRICS_NOT_UPSTREAM = METRICS_KMEANS[:3] + NN_METRICS + METRICS_KMEANS[3:]


CLUSTER_METRICS = METRICS_KMEANS                                                         # --cluster_metrics computes these


def evaluate(writer, real, collection, baseline, valid_real, compute_final_only=False, seed=1, nn_metrics=False, nn_k=3,
             cluster_metrics=False, prd_clusters=20, prd_runs=10, ndb_bins=50):
    """sample_ncsn.py:69-186: the distance metrics of utils/metrics.py between the eval set ``real`` and 20 points of the
    sampler's ``collection`` (T, N, *shape), the ``baseline`` (None: skipped), and two controls: ``random`` (standard normals
    of the sample shape, drawn from a generator seeded by ``seed`` -- unseeded upstream) and ``real`` (``valid_real`` against
    the eval set).  Scalars go to ``writer`` as {model}/{frechet_distance,mmd_rbf,mmd_polynomial} with step = i.

    Definitions this port fixes: an (N, S, C) set is evaluated as N*S frames of C (upstream hands 3-D
    arrays to np.cov, which raises); the returned stats are the final ``ncsn`` point (upstream: whatever the last loop
    iteration left, the real-vs-real control).  The precision/recall, realism and NDB metrics of the reference's evaluate()
    are not defined in its utils/metrics.py.  ``nn_metrics``: additionally {model}/{improved_precision,improved_recall,
    improved_f1,ipr_realism} as DESIGN.md section 14 defines them (radius = distance to the ``nn_k``-th neighbour), for the same
    points and steps, and the same four keys in the returned stats.  ``cluster_metrics``: additionally {model}/{precision,
    recall,f1,ndb}, the reference's tags (:144-146,160), as DESIGN.md section 15 defines them -- the PRD histogram on
    ``prd_clusters`` clusters averaged over ``prd_runs`` k-means runs and NDB on ``ndb_bins`` bins, all seeded by ``seed`` -- and
    the same four keys in the returned stats.  Without it the k-means metrics are not computed."""
    from smd_amd import metrics as M
    assert tuple(collection.shape[1:]) == tuple(real.shape), (collection.shape, real.shape)
    lo, hi = float(collection[-1].min()), float(collection[-1].max())
    log.info(f"Generated sample range: [{lo}, {hi}]")
    log.info(f"Test sample range: [{float(real.min())}, {float(real.max())}]")
    if lo < -1.0 or hi > 1.0 or real.min() < -1 or real.max() > 1.0:
        log.warning("Normalize test samples and generated samples to [-1, 1] range.")

    gen_test_points = [collection[int(i)] for i in np.linspace(0, len(collection) - 1, 20).astype(np.uint32)]
    if compute_final_only:
        gen_test_points = [gen_test_points[-1]]
    random_points = [np.random.default_rng(seed).standard_normal(tuple(collection[0].shape)).astype(np.float32)]
    real_points = [valid_real]              # valid_real is real (the driver's call): the symmetric path, sklearn's X is Y

    ref = M.ReferenceSet(real, collection.device if torch.is_tensor(collection) and collection.is_cuda else None)
    stats = {}
    for model, test_points in [("baseline", [baseline]), ("ncsn", gen_test_points), ("random", random_points),
                               ("real", real_points)]:
        if any(point is None for point in test_points):
            continue
        for i, samples in enumerate(test_points):
            frechet_dist = M.frechet_distance(ref, samples)
            mmds = M.kernel_mmds(ref, samples)
            writer.scalar(f"{model}/frechet_distance", frechet_dist, step=i)
            writer.scalar(f"{model}/mmd_rbf", mmds["mmd_rbf"], step=i)
            writer.scalar(f"{model}/mmd_polynomial", mmds["mmd_polynomial"], step=i)
            if model == "ncsn":
                stats = {"frechet_dist": frechet_dist, "mmd_rbf": mmds["mmd_rbf"], "mmd_polynomial": mmds["mmd_polynomial"]}
            if nn_metrics:
                nn = M.improved_metrics(ref, samples, nn_k)
                for name in NN_METRICS:
                    writer.scalar(f"{model}/{name}", nn[name], step=i)
                if model == "ncsn":
                    stats.update(nn)
            if cluster_metrics:
                km = M.cluster_metrics(ref, samples, prd_clusters, prd_runs, ndb_bins, seed)
                for name in CLUSTER_METRICS:
                    writer.scalar(f"{model}/{name}", km[name], step=i)
                if model == "ncsn":
                    stats.update(km)
    writer.flush()
    return stats


def check_cluster_flags(FLAGS):
    """the refusals of --cluster_metrics, before the GPU is touched"""
    if FLAGS.interpolate:
        raise SystemExit("--cluster_metrics does not apply to --interpolate: there is no collection of the sample shape to compare "
                         "with the eval set")
    if not FLAGS.compute_metrics:
        raise SystemExit("--cluster_metrics adds the k-means metrics to the evaluation: it needs --compute_metrics")
    for name, lo, hi in (("prd_clusters", 2, 128), ("prd_runs", 1, 100), ("ndb_bins", 2, 128)):
        v = getattr(FLAGS, name)
        if v is None or not lo <= v <= hi:
            raise SystemExit(f"--{name}={v}: --cluster_metrics takes {name} from {lo} to {hi}")
    shape = [int(v) for v in FLAGS.data_shape]
    frames = (FLAGS.sample_size or 0) * (int(np.prod(shape[:-1])) if len(shape) > 1 else 1)
    k = max(FLAGS.prd_clusters, FLAGS.ndb_bins)
    if frames < k:
        raise SystemExit(f"--cluster_metrics: --sample_size={FLAGS.sample_size} examples of shape {tuple(shape)} are {frames} frames, "
                         f"fewer than the {k} clusters of --prd_clusters={FLAGS.prd_clusters} / --ndb_bins={FLAGS.ndb_bins}")


def check_ddim_flags(FLAGS, walk=None):
    """the refusals of --ddim_steps / --ddim_eta / --ddim_encode / --ddim_order / --ddim_spacing / --ddim_solver, before the GPU is touched;
    ``walk``: the recorded walk of a distilled checkpoint (resolve_distill_walk), whose length --ddim_steps then is"""
    used = [f"--{n}" for n in ("ddim_steps", "ddim_eta", "ddim_encode") if FLAGS.is_present(n) and getattr(FLAGS, n)]
    used += [f"--{n}" for n, off in (("ddim_order", 1), ("ddim_spacing", "uniform"), ("ddim_solver", "default"))
             if FLAGS.is_present(n) and getattr(FLAGS, n) != off]
    if used and FLAGS.sampling != "ddpm":
        raise SystemExit(f"{', '.join(used)}: the strided sampler walks a DDPM schedule, it needs --sampling=ddpm (got --sampling={FLAGS.sampling})")
    steps = FLAGS.ddim_steps
    if walk is None and (steps is None or not (steps == 0 or 2 <= steps <= FLAGS.num_sigmas)):
        raise SystemExit(f"--ddim_steps={steps}: 0 (every timestep) or from 2 to --num_sigmas={FLAGS.num_sigmas} timesteps")
    if FLAGS.ddim_eta < 0:
        raise SystemExit(f"--ddim_eta={FLAGS.ddim_eta}: the noise scale is >= 0")
    if (FLAGS.ddim_eta or FLAGS.ddim_encode) and not steps:
        raise SystemExit("--ddim_eta / --ddim_encode belong to the strided sampler: give --ddim_steps")
    if FLAGS.ddim_encode and not FLAGS.interpolate:
        raise SystemExit("--ddim_encode replaces the encoder of --interpolate: it needs --interpolate")
    order, spacing = FLAGS.ddim_order, FLAGS.ddim_spacing
    if order not in (1, 2):
        raise SystemExit(f"--ddim_order={order}: 1 (the strided update, DDIM) or 2 (DPM-Solver++(2M))")
    if (order != 1 or spacing != "uniform") and not steps:
        raise SystemExit("--ddim_order / --ddim_spacing belong to the strided sampler: give --ddim_steps")
    if order == 2 and FLAGS.ddim_eta != 0:
        raise SystemExit(f"--ddim_order=2 is a deterministic solver: it needs --ddim_eta=0 (got --ddim_eta={FLAGS.ddim_eta})")
    if order == 2 and FLAGS.ddim_encode:
        raise SystemExit("--ddim_order=2 with --ddim_encode: the inversion is first order, so encoding and decoding would not be the "
                         "same solver; use --ddim_order=1 or the stochastic encoder")
    if order == 2 and spacing == "uniform":
        log.warning("--ddim_order=2 --ddim_spacing=uniform: on a grid that is uniform in t the second-order update is LESS accurate "
                    "than --ddim_order=1 at the same --ddim_steps (history weight up to 3.7; DESIGN.md section 18, the table): "
                    "use --ddim_spacing=logsnr")
    solver = FLAGS.ddim_solver
    if solver != "default":
        flag = f"--ddim_solver={solver}"
        if not steps:
            raise SystemExit(f"{flag} belongs to the strided sampler: give --ddim_steps (or a distilled checkpoint, which records its walk)")
        if order == 2:
            raise SystemExit(f"{flag} with --ddim_order=2: these are two solvers; leave --ddim_order at 1")
        if FLAGS.ddim_eta != 0:
            raise SystemExit(f"{flag} is a deterministic solver: it needs --ddim_eta=0 (got --ddim_eta={FLAGS.ddim_eta})")
        if FLAGS.ddim_encode:
            raise SystemExit(f"{flag} with --ddim_encode: the inversion is first order, so encoding and decoding would not be the "
                             "same solver; use --ddim_solver=default or the stochastic encoder")
        if FLAGS.analytic_variance != "none":
            raise SystemExit(f"{flag} with --analytic_variance={FLAGS.analytic_variance}: the solver is deterministic, it has no "
                             "noise term to give a variance to")
        if spacing == "uniform" and walk is None:
            log.warning("%s --ddim_spacing=uniform: on a grid that is uniform in t every higher-order update is LESS accurate than "
                        "--ddim_order=1 at the same --ddim_steps (DESIGN.md section 29, the table): use --ddim_spacing=logsnr", flag)


def check_bound_flags(FLAGS):
    """the refusals of --compute_bound / --bound_steps / --bound_only, before the GPU is touched"""
    if not FLAGS.compute_bound:
        used = [f"--{n}" for n in ("bound_steps", "bound_only") if FLAGS.is_present(n) and getattr(FLAGS, n)]
        if used:
            raise SystemExit(f"{', '.join(used)}: options of the variational bound, give --compute_bound")
        return
    if FLAGS.sampling != "ddpm":
        raise SystemExit(f"--compute_bound: the variational bound is that of a DDPM schedule, it needs --sampling=ddpm (got --sampling={FLAGS.sampling})")
    if FLAGS.loss != "ddpm":
        raise SystemExit(f"--compute_bound: the network must be an eps-predictor trained with --loss=ddpm (got --loss={FLAGS.loss})")
    steps = FLAGS.bound_steps
    if steps is None or not (steps == 0 or 2 <= steps <= FLAGS.num_sigmas):
        raise SystemExit(f"--bound_steps={steps}: 0 (every timestep) or from 2 to --num_sigmas={FLAGS.num_sigmas} timesteps")


def check_analytic_flags(FLAGS, world=1):
    """the refusals of --analytic_variance / --analytic_examples / --analytic_draws / --analytic_moments, before the GPU is touched
    (after resolve_distill_walk: a recorded walk has set --ddim_steps)"""
    if FLAGS.analytic_variance == "none":
        used = [f"--{n}" for n in ("analytic_examples", "analytic_draws", "analytic_moments") if FLAGS.is_present(n)]
        if used:
            raise SystemExit(f"{', '.join(used)}: options of the analytic variance, give --analytic_variance=scalar or element")
        return
    flag = f"--analytic_variance={FLAGS.analytic_variance}"
    if FLAGS.sampling != "ddpm":
        raise SystemExit(f"{flag}: the optimal variance is that of a DDPM schedule, it needs --sampling=ddpm (got --sampling={FLAGS.sampling})")
    if not FLAGS.ddim_steps:
        raise SystemExit(f"{flag} belongs to the strided sampler: give --ddim_steps (or a distilled checkpoint, which records its "
                         "walk); the every-timestep walk is --ddim_steps=--num_sigmas")
    if FLAGS.ddim_order == 2:
        raise SystemExit(f"{flag} with --ddim_order=2: the second-order solver is deterministic, it has no noise term to give a variance to")
    if world > 1:
        raise SystemExit(f"{flag} runs in a single process (the estimate is not sharded): got WORLD_SIZE={world}")
    if FLAGS.analytic_variance == "element" and FLAGS.compute_bound:
        raise SystemExit(f"{flag} with --compute_bound: the bound takes the scalar form only (per-element variances would need "
                         "per-element sums); use --analytic_variance=scalar")
    if FLAGS.analytic_examples is None or FLAGS.analytic_examples < 1:
        raise SystemExit(f"--analytic_examples={FLAGS.analytic_examples}: {flag} estimates on at least one example")
    if FLAGS.analytic_draws is None or FLAGS.analytic_draws < 1:
        raise SystemExit(f"--analytic_draws={FLAGS.analytic_draws}: {flag} takes at least one draw per example")
    if FLAGS.analytic_moments and not os.path.isfile(os.path.expanduser(FLAGS.analytic_moments)):
        raise SystemExit(f"--analytic_moments={FLAGS.analytic_moments}: no such file")


def analytic_moments(FLAGS, model, sigmas, walk, examples, bound_timesteps=None):
    """--analytic_variance: the statistic g for every timestep the run needs -- the sampling walk and, with --compute_bound, the
    bound's timesteps -- loaded from --analytic_moments or estimated on ``examples`` (a callable returning them, model space)
    and written to {sampling_dir}/ncsn/analytic_moments.safetensors.  Returns (g [K][...], timesteps [K] ascending)."""
    from smd_amd import analytic as A
    from smd_amd import ncsn
    want = A.run_metadata(FLAGS, _prediction(FLAGS), model.engine)
    taus = A.resolve_walk(FLAGS, sigmas, walk)
    need = np.unique(np.concatenate([taus] + ([np.asarray(bound_timesteps, dtype=np.int64)] if bound_timesteps is not None else [])))
    shape = tuple(model.engine.cfg.sample_shape)
    if FLAGS.analytic_moments:
        path = os.path.expanduser(FLAGS.analytic_moments)
        try:
            g, ts, count, meta = A.load_moments(path)
            A.check_moments(path, g, ts, meta, want, need, shape)
        except ValueError as e:
            raise SystemExit(str(e))
        log.info("analytic variance: loaded E[eps_hat^2] at %d timesteps (%d example-draws) from %s", len(ts), count, path)
        return g, ts
    t0 = time.time()
    x0 = np.ascontiguousarray(examples(), dtype=np.float32)
    rng = ncsn.split(ncsn.make_key(FLAGS.sample_seed, "philox"), num=5)[4]
    g, count = ncsn.estimate_score_moments(model, sigmas, x0, need, draws=FLAGS.analytic_draws, rng=rng,
                                           batch=min(256, len(x0)), prediction=_prediction(FLAGS), use_graph=FLAGS.graph)
    model.drop_sampler_cache()
    A.save_moments(os.path.join(FLAGS.sampling_dir, "ncsn", A.MOMENTS_FILE), g, need, count,
                   dict(want, examples=str(len(x0)), draws=str(FLAGS.analytic_draws),
                        example_source="synthetic" if FLAGS.synthetic else "dataset"))
    log.info("analytic variance: E[eps_hat^2] at %d timesteps from %d examples x %d draws in %.1f s (mean %.4f)", len(need), len(x0),
             FLAGS.analytic_draws, time.time() - t0, float(np.clip(g, 0, 1).mean()))
    return g, need


def check_copy_flags(FLAGS):
    """the refusals of --copy_metrics / --copy_k / --copy_train_examples, before the GPU is touched"""
    if not FLAGS.copy_metrics:
        return
    if FLAGS.interpolate:
        raise SystemExit("--copy_metrics does not apply to --interpolate: its output holds 9 interpolation points per sample, not a "
                         "set of the sample shape to search the training set for")
    if FLAGS.copy_k is None or not 1 <= FLAGS.copy_k <= 8:
        raise SystemExit(f"--copy_k={FLAGS.copy_k}: --copy_metrics keeps from 1 to 8 training neighbours per row")
    if FLAGS.copy_train_examples is None or FLAGS.copy_train_examples < 0:
        raise SystemExit(f"--copy_train_examples={FLAGS.copy_train_examples}: 0 (every training example) or the number of examples to search")


COPY_SYNTHETIC_SEED = 4322         # --synthetic --copy_metrics: the training set's seed; the eval examples ("real") take 4321
COPY_SLAB_EXAMPLES = 1024         # training examples per slab of the search: 64 MiB of fp32 at the base shape (32, 512)


def copy_metrics_report(FLAGS, train, real, generated, dev):
    """--copy_metrics: the nearest training neighbours of the ``generated`` examples next to those of the eval examples ``real``,
    at frame and at sequence level (smd_amd.metrics.copy_metrics).  ``train``: the training examples in
    the normalised space the model sees, on the host; they are searched in slabs of COPY_SLAB_EXAMPLES.  Writes
    {sampling_dir}/ncsn/copy_report.json (the scalars, k, the set sizes, the definitions' version) and nearest_train.pkl (per
    generated example the k nearest training sequences and per frame the nearest training frame), logs the scalars under copy/..."""
    import json

    from smd_amd import data, train_utils
    from smd_amd import metrics as M
    t0 = time.time()
    k = FLAGS.copy_k
    n = len(generated)
    frames = int(np.prod(generated.shape[1:-1])) if generated.ndim > 2 else 1
    as3 = lambda a: np.ascontiguousarray(a, dtype=np.float32).reshape(len(a), frames, -1)
    train, real, generated = as3(train), as3(real), as3(generated)
    slabs = [train[i:i + COPY_SLAB_EXAMPLES] for i in range(0, len(train), COPY_SLAB_EXAMPLES)]
    rep = M.copy_metrics(slabs, real, generated, k, device=dev)
    scalars = {name + s: rep[name + s] for s in ("", "_seq") for name in M.COPY_SCALARS}
    summary = dict(scalars, k=k, version=rep["version"], num_train_examples=int(len(train)), num_generated=int(n),
                   num_held_out=int(len(real)), frames_per_example=frames,
                   **{name + s: int(rep[name + s]) for s in ("", "_seq") for name in ("n_train", "n_fake", "n_held_out")})
    out_dir = os.path.join(FLAGS.sampling_dir, "ncsn")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "copy_report.json"), "w") as f:
        json.dump(summary, f, indent=1)
    fi = rep["nn_idx"][:, 0].reshape(n, frames)
    data.save(dict(k=k, sequence_example=rep["nn_idx_seq"], sequence_distance=np.sqrt(rep["nn_d2_seq"].astype(np.float64)),
                   frame_example=fi // frames, frame_index=fi % frames,
                   frame_distance=np.sqrt(rep["nn_d2"][:, 0].astype(np.float64)).reshape(n, frames)),
              os.path.join(out_dir, "nearest_train.pkl"))
    train_utils.log_metrics({f"copy/{name}": v for name, v in scalars.items()}, 1, 1)
    log.info("copy metrics: %d generated and %d eval examples against %d training examples (k = %d) in %.1f s", n, len(real),
             len(train), k, time.time() - t0)


def compute_bound(FLAGS, model, real, lo, hi, sigmas, rank, world, analytic_g=None):
    """The variational bound over this rank's rows [lo, hi) of the eval set; rank 0 gathers and writes
    {sampling_dir}/ncsn/bound.json (scalars, per-timestep means) and bound_terms.pkl (the per-example arrays)."""
    import json

    from smd_amd import data, ncsn
    rng = ncsn.split(ncsn.make_key(FLAGS.sample_seed, FLAGS.rng_impl), num=4)[3]
    t0 = time.time()
    out = ncsn.variational_bound(rng, model, sigmas, np.ascontiguousarray(real[lo:hi], dtype=np.float32), FLAGS.bound_steps,
                                 sample_offset=lo, global_num_samples=len(real), use_graph=FLAGS.graph,
                                 prediction=_prediction(FLAGS), analytic=analytic_g)
    model.drop_sampler_cache()
    parts = [out]
    if world > 1:
        import torch.distributed as dist
        parts = [None] * world
        dist.gather_object(out, parts if rank == 0 else None, dst=0)
    if rank != 0:
        return
    terms = np.concatenate([p["terms"] for p in parts], axis=1)
    # sum (eps - out)^2 means nothing when the network's output is x0 or v: variational_bound then returns None for it
    eps_mse = np.concatenate([p["eps_mse"] for p in parts], axis=1) if out["eps_mse"] is not None else None
    prior = np.concatenate([p["prior"] for p in parts])
    exact = out["total"] is not None
    total = np.concatenate([p["total"] for p in parts]) if exact else None
    per = int(np.prod(real.shape[1:]))
    nats = float(total.mean() / per) if exact else None
    bits = float(total.mean() / (per * np.log(2.0))) if exact else None
    summary = dict(nats_per_dim=nats, bits_per_dim=bits, total=float(total.mean()) if exact else None, prior=float(prior.mean()),
                   timesteps=[int(t) for t in out["timesteps"]], terms=[float(v) for v in terms.mean(axis=1)],
                   eps_mse=None if eps_mse is None else [float(v) for v in eps_mse.mean(axis=1)], dtype=FLAGS.dtype, num_examples=int(len(real)), clip=1.0,
                   var_0=float(out["var_0"]), exact=bool(exact))
    if out.get("prediction", "eps") != "eps":               # an x0 / v model says so (and has eps_mse: null); eps files are as ever
        summary["prediction"] = out["prediction"]
    if analytic_g is not None:                              # single process (check_analytic_flags): out is the whole eval set
        summary.update(analytic_terms=[float(v) for v in out["analytic_terms"].mean(axis=1)],
                       analytic_total=float(out["analytic_total"].mean()), analytic_bits_per_dim=float(out["analytic_bits_per_dim"]),
                       sigma2_ratio=[float(v) for v in out["sigma2_ratio"]])
    log_dir = FLAGS.sampling_dir
    os.makedirs(os.path.join(log_dir, "ncsn"), exist_ok=True)
    with open(os.path.join(log_dir, "ncsn/bound.json"), "w") as f:
        json.dump(summary, f, indent=1)
    data.save(dict(timesteps=out["timesteps"], terms=terms, eps_mse=eps_mse, prior=prior, total=total),
              os.path.join(log_dir, "ncsn/bound_terms.pkl"))
    log.info("variational bound on %d examples (%s, %d timesteps, %.1f s): %s, prior %.4f nats", len(real), FLAGS.dtype,
             len(out["timesteps"]), time.time() - t0,
             f"{bits:.4f} bits/dim ({nats:.4f} nats/dim)" if exact else "a sub-sequence of the timesteps, no total", prior.mean())


def main(argv):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    FLAGS = F.make_flags(include_sample=True)
    FLAGS.parse(argv[1:])
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if rank == 0:
        log.info(FLAGS.flags_into_string())
    if FLAGS.sampling not in ("ddpm", "ald", "cas"):
        raise SystemExit(f"Unknown sampling algorithm: {FLAGS.sampling}")
    if FLAGS.interpolate and FLAGS.sampling != "ddpm":
        raise SystemExit("--interpolate is a DDPM mode (sample_ncsn.py:250,270 assert it)")
    if FLAGS.compute_metrics and FLAGS.interpolate:
        raise SystemExit("--compute_metrics does not apply to --interpolate: its collection holds 9 interpolation points per "
                         "sample, not the sample shape evaluate() compares with the eval set (sample_ncsn.py:92 asserts it)")
    if FLAGS.nn_metrics and FLAGS.interpolate:
        raise SystemExit("--nn_metrics does not apply to --interpolate: there is no collection of the sample shape to compare "
                         "with the eval set")
    if FLAGS.nn_metrics and not FLAGS.compute_metrics:
        raise SystemExit("--nn_metrics adds the nearest-neighbour metrics to the evaluation: it needs --compute_metrics")
    if FLAGS.nn_metrics and not 1 <= FLAGS.nn_k <= 8:
        raise SystemExit(f"--nn_k={FLAGS.nn_k}: the radius is the distance to the k-th neighbour for k from 1 to 8")
    if FLAGS.cluster_metrics:
        check_cluster_flags(FLAGS)
    walk = resolve_distill_walk(FLAGS)
    if walk is not None and rank == 0:
        log.info("distilled checkpoint: sampling on its walk of %d timesteps %s", len(walk), walk)
    check_ddim_flags(FLAGS, walk)
    check_bound_flags(FLAGS)
    check_copy_flags(FLAGS)
    check_analytic_flags(FLAGS, world)
    try:
        FLAGS.prediction = resolve_prediction_flag(FLAGS)
    except ValueError as e:
        raise SystemExit(str(e))
    if rank == 0:
        log.info("prediction: %s", FLAGS.prediction)
    torch.cuda.set_device(local_rank)
    dev = f"cuda:{local_rank}"
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device(dev))
    from smd_amd import data, ncsn
    from smd_amd.trainer import shard_bounds
    from train_ncsn import build_datasets, log_langevin_dynamics, model_shape

    slice_idx = data.load(os.path.expanduser(FLAGS.slice_ckpt)) if FLAGS.slice_ckpt else None
    dim_weights = data.load(os.path.expanduser(FLAGS.dim_weights_ckpt)) if FLAGS.dim_weights_ckpt else None
    shape = model_shape(FLAGS, slice_idx)
    sigmas = schedule.create_noise_schedule(FLAGS.sigma_begin, FLAGS.sigma_end, FLAGS.num_sigmas,
                                            schedule=FLAGS.schedule_type)
    # "real" examples: the reference needs the eval set even for unconditional sampling (:387-402)
    if FLAGS.synthetic:
        n = FLAGS.sample_size
        real = data.SyntheticLatents(shape, max(n, 1), max(n, 1), 4321).take_examples(n)
        tmin, tmax, emin, emax = -1.0, 1.0, -1.0, 1.0
        if FLAGS.copy_metrics and rank == 0:                                # no dataset here: a training set of the same law
            n_train = max(FLAGS.copy_train_examples or n, 2)
            copy_train = data.SyntheticLatents(shape, n_train, n_train, COPY_SYNTHETIC_SEED).take_examples(n_train)
    else:
        train_ds, eval_ds, _, _ = build_datasets(FLAGS, shape, None, 0, 1)
        real = eval_ds.take_examples(FLAGS.sample_size)
        tmin, tmax, emin, emax = train_ds.min, train_ds.max, eval_ds.min, eval_ds.max
        if FLAGS.copy_metrics and rank == 0:
            copy_train = train_ds.take_examples(FLAGS.copy_train_examples or len(train_ds.array))
    num = len(real)
    lo, hi = shard_bounds(num, world, rank)
    model, rng = load_model(FLAGS, shape, dev)

    analytic = None
    bound_g = None
    if FLAGS.analytic_variance != "none":
        def analytic_examples():                        # the training split as --copy_metrics reads it, else the eval examples
            n = FLAGS.analytic_examples
            if FLAGS.synthetic:
                return data.SyntheticLatents(shape, n, n, COPY_SYNTHETIC_SEED).take_examples(n)
            src = train_ds if len(getattr(train_ds, "array", ())) else eval_ds
            return src.take_examples(min(n, len(src.array)))
        bound_ts = None
        if FLAGS.compute_bound:
            bound_ts = np.arange(FLAGS.num_sigmas) if FLAGS.bound_steps == 0 else schedule.stride_timesteps(FLAGS.num_sigmas, FLAGS.bound_steps)
        from smd_amd import analytic as A
        g_all, g_ts = analytic_moments(FLAGS, model, sigmas, walk, analytic_examples, bound_ts)
        taus = A.resolve_walk(FLAGS, sigmas, walk)
        analytic = (FLAGS.analytic_variance, g_all[np.searchsorted(g_ts, taus)])
        if bound_ts is not None:
            bound_g = g_all[np.searchsorted(g_ts, np.unique(bound_ts))]

    if FLAGS.compute_bound:
        compute_bound(FLAGS, model, real, lo, hi, sigmas, rank, world, analytic_g=bound_g)
        if FLAGS.bound_only:
            if world > 1:
                import torch.distributed as dist
                dist.destroy_process_group()
            return

    if FLAGS.infill:                                                        # :405-423
        samples = np.copy(real[lo:hi])
        masks = np.zeros(samples.shape, np.float32)
        if len(shape) == 1:
            samples[:, shape[0] // 2:] = 0
            masks[:, :shape[0] // 2] = 1
        else:
            idx = list(range(shape[0]))
            fixed_idx, infilled_idx = idx[:8] + idx[-8:], idx[8:-8]
            samples[:, infilled_idx, :] = 0
            masks[:, fixed_idx, :] = 1
        generated, collection, ld_metrics = infill_samples(FLAGS, model, rng, samples, masks, sigmas, sample_offset=lo,
                                                           global_num_samples=num, walk=walk, analytic=analytic)
    elif FLAGS.interpolate:                                                 # :425-435
        generated, collection, ld_metrics = interpolate_samples(model, sigmas, real, lo, hi, rng, FLAGS.sample_seed, FLAGS.rng_impl,
                                                                dev, FLAGS.graph, ddim_steps=FLAGS.ddim_steps,
                                                                ddim_eta=FLAGS.ddim_eta, ddim_encode=FLAGS.ddim_encode,
                                                                ddim_order=FLAGS.ddim_order, ddim_spacing=FLAGS.ddim_spacing,
                                                                prediction=FLAGS.prediction, walk=walk, analytic=analytic,
                                                                ddim_solver=FLAGS.ddim_solver)
    else:                                                                   # :437-439
        generated, collection, ld_metrics = generate_samples(FLAGS, model, rng, shape, hi - lo, sigmas, sample_offset=lo,
                                                             global_num_samples=num, walk=walk, analytic=analytic)

    # evaluate() reads the device collection where there is one (a single rank); the shards of several ranks are gathered
    # on the host below
    coll_dev = collection if FLAGS.compute_metrics and world == 1 and torch.is_tensor(collection) else None
    generated = generated.cpu().numpy() if torch.is_tensor(generated) else generated
    collection = collection.cpu().numpy() if torch.is_tensor(collection) else collection
    if world > 1:                                                           # host-side gather of the shards
        import torch.distributed as dist
        gathered = [None] * world
        dist.gather_object((generated, collection), gathered if rank == 0 else None, dst=0)
        if rank == 0:
            axis = 1 if FLAGS.interpolate else 0
            generated = np.concatenate([g for g, _ in gathered], axis=axis)
            collection = np.concatenate([c for _, c in gathered], axis=axis + 1)

    if rank == 0 and FLAGS.flush:                                           # :452-471
        log_dir = FLAGS.sampling_dir
        pca = data.load(os.path.expanduser(FLAGS.pca_ckpt)) if FLAGS.pca_ckpt else None       # :380-381
        inv = lambda b, mn, mx: data.inverse_data_transform(b, FLAGS.normalize, pca, mn, mx, slice_idx, dim_weights)
        if not FLAGS.interpolate:
            data.save(inv(collection, tmin, tmax), os.path.join(log_dir, "ncsn/collection.pkl"))
        data.save(inv(real, emin, emax), os.path.join(log_dir, "ncsn/real.pkl"))
        data.save(inv(generated, tmin, tmax), os.path.join(log_dir, "ncsn/generated.pkl"))
    if rank == 0 and FLAGS.compute_metrics:                                 # :473-476, independent of --flush
        from smd_amd import train_utils
        log_dir = FLAGS.sampling_dir
        log_langevin_dynamics(ld_metrics, 0, log_dir)
        if FLAGS.cluster_metrics and not FLAGS.nn_metrics:
            log.warning("--compute_metrics: %s of the reference's evaluate() call functions that utils/metrics.py does not define "
                        "and are not computed (--nn_metrics); %s are computed as DESIGN.md section 15 defines them (%d clusters x %d "
                        "runs, %d bins)", ", ".join(NN_METRICS), ", ".join(CLUSTER_METRICS), FLAGS.prd_clusters, FLAGS.prd_runs,
                        FLAGS.ndb_bins)
        elif FLAGS.cluster_metrics:
            pass                                                            # every scalar of the reference's evaluate() is computed
        elif FLAGS.nn_metrics:
            log.warning("--compute_metrics: %s of the reference's evaluate() call functions that utils/metrics.py does not define "
                        "and are not computed; %s are computed as DESIGN.md section 14 defines them (k = %d)",
                        ", ".join(METRICS_KMEANS), ", ".join(NN_METRICS), FLAGS.nn_k)
        else:
            log.warning("--compute_metrics: %s of the reference's evaluate() call functions that utils/metrics.py does not define; "
                        "only frechet_distance, mmd_rbf and mmd_polynomial are computed", ", ".join(METRICS_NOT_UPSTREAM))
        writer = train_utils.JsonlWriter(log_dir)
        stats = evaluate(writer, real, collection if coll_dev is None else coll_dev, None, real,
                         compute_final_only=FLAGS.compute_final_only, seed=FLAGS.sample_seed, nn_metrics=FLAGS.nn_metrics,
                         nn_k=FLAGS.nn_k, cluster_metrics=FLAGS.cluster_metrics, prd_clusters=FLAGS.prd_clusters,
                         prd_runs=FLAGS.prd_runs, ndb_bins=FLAGS.ndb_bins)
        writer.close()
        train_utils.log_metrics(stats, 1, 1)
    if rank == 0 and FLAGS.copy_metrics:                                    # on the final samples only, with or without --compute_metrics
        copy_metrics_report(FLAGS, copy_train, real, generated, dev)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv)
