"""GPU box: host + device time of srk_ba_upload_scene by stage (SRK_DEBUG trace), first and second upload of a handle."""
import os, sys, time
os.environ["SRK_DEBUG"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import surikatoko_amd as sa
name = sys.argv[1] if len(sys.argv) > 1 else "C3_1kcam_100kpt"
if name == "all_visible_60":
    spec = sa.SceneSpec(n_frames=60, grid_nx=81, grid_ny=41, vis_window=0); sc = sa.generate_scene(spec); f0 = spec.f0
else:
    sc = sa.config_scene(name); f0 = sa.CONFIGS[name].f0
ba = sa.BundleAdjustmentKanatani(0)
if len(sys.argv) > 2 and sys.argv[2] == "factors":  # the chain of tools/relpose_rate.py and the 60 sets of tools/jointprior_rate.py
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import jointprior_rate, relpose_rate
    from surikatoko_amd import ba as B
    fs = relpose_rate.factor_set(B, sc, "chain")
    ba.set_relative_pose_factors(fs[0], fs[1], fs[2], info=fs[3])
    ba.set_joint_pose_priors(jointprior_rate.prior_sets(sc, "60_sets_of_16_chained"))
for k in range(int(sys.argv[3]) if len(sys.argv) > 3 else 3):
    t = time.perf_counter(); assert ba.upload(f0, sc); print("upload", k, "%.1f ms" % ((time.perf_counter() - t) * 1e3), file=sys.stderr, flush=True)
