"""Worker of tests/test_gpu_information.py::test_two_ranks_on_one_gpu_match_world_size_one: one process per rank, all on
cuda:0, gloo backend.  The landmark-sharded LM loop with a Huber loss and per-observation information, each rank passing its
shard's slice of the values; stores this rank's result, its observations' weights and residuals."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def scene(spec_kwargs):
    """(scene, information)"""
    import surikatoko_amd as sa
    import robust_ref as rr
    import weighted_ref as wr
    sc = sa.generate_scene(sa.SceneSpec(**spec_kwargs))
    rr.inject_outliers(sc, 0.05, 20, 60, seed=13)
    return sc, wr.make_information(sc, seed=17)


def run(rank, world, out_dir, spec_kwargs, iters):
    import torch.distributed as dist
    import surikatoko_amd as sa
    from surikatoko_amd.ba import revert_normalization
    from surikatoko_amd.dist import make_allreduce_hook

    dist.init_process_group(backend="gloo", rank=rank, world_size=world,
                            init_method="file://" + os.path.join(out_dir, "rendezvous"))
    try:
        full, q = scene(spec_kwargs)
        ok, nrm = sa.normalize_scene_inplace(full)
        assert ok
        shard, (lo, hi) = full.shard(rank, world)
        o0, o1 = int(full.row_ptr[lo]), int(full.row_ptr[hi])
        ba = sa.BundleAdjustmentKanatani(0)
        ba.set_allreduce(make_allreduce_hook(None, "cuda:0"), rank, world)
        ba.set_robust_loss("huber", 2.0)
        ba.set_observation_information(q[o0:o1])  # the shard's own values
        assert ba.upload(600.0, shard, already_normalized=True)
        crit = sa.BundleAdjustmentKanataniTermCriteria()
        crit.AllowedReprojErrRelativeChange(1e-7)
        ok = ba.optimize(crit, iters)
        w = ba.observation_weights()
        e = ba.observation_residuals()
        out = shard.copy()
        ba.download(out, revert_normalization=False)
        revert_normalization(out, nrm)
        r = ba.report
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ok=ok, lo=lo, hi=hi, points=out.points, cam_R=out.cam_R,
                 cam_T=out.cam_T, iterations=r.iterations, attempts=r.attempts, err_initial=r.err_initial,
                 err_final=r.err_final, weights=w, residuals=e)
        ba.close()
    finally:
        dist.destroy_process_group()
