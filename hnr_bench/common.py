"""Shared pieces of the benchmark: arguments, rank spawning, the synthetic scene, one frame through the renderer,
profile lookup."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
F32_MFMA_PEAK_TF = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
BF16_MFMA_PEAK_TF = 2500.0     # MI355X_MICROARCH.md: bf16 MFMA dense peak (v_mfma_f32_32x32x16_bf16)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=float, default=2.0e6)
    ap.add_argument("--chunk", type=int, default=0, help="rays per launch (0 = the whole frame in one launch)")
    ap.add_argument("--scene", default="scene0241")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--margin", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-train-leg", action="store_true")
    ap.add_argument("--train-sharded-only", action="store_true", help="of the training legs run only the C5 "
                                                                      "patch-sharded step "
                                                                      "(tools/predict_train_scaling.sh)")
    ap.add_argument("--no-f32-anchor", action="store_true", help="skip the one fp32-MFMA frame rendered beside the "
                                                                 "timed region (fp32_mfma_anchor)")
    ap.add_argument("--cpu-sample-rays", type=int, default=2304)
    ap.add_argument("--shard", choices=("lines", "blocks"), default="lines",
                    help="strong scaling: scan lines dealt round-robin to the ranks (balanced: busiest rank 1.01x the "
                         "mean work at N = 8) or N "
                         "contiguous blocks of scan lines (the reference's chunk order; busiest block 1.68x the mean "
                         "on this frame)")
    ap.add_argument("--knn-order", choices=("sorted", "reference"), default=None,
                    help="neighbour order of the query; default: whatever the library ships (HybridRenderer.knn_order "
                         "= 'reference': slot for slot "
                         "the reference's insertion history, the order the training path uses too).  sorted = the "
                         "reference's neighbour SETS in "
                         "ascending (d2, enumeration) order (hnr_query_params.knn_order = 1), an opt-in A/B")
    ap.add_argument("--band", type=int, default=1, help="--shard lines: scan lines per dealt band")
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong",
                    help="strong: the N ranks share ONE fixed frame (north_star); weak: one whole frame per rank")
    ap.add_argument("--dump-colors", default="", help="rank 0 writes the assembled [R,3] colours of the last step to "
                                                      "this .npy file")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes what the last timed step returned to DIR/<name>.npy (frame.dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything reported beside the headline: the other shard order (N > 1), the training "
                         "legs, the rooflines, the amortised / resident figures, the fp32-MFMA anchor frame and the CPU "
                         "baseline (each still subject to its --no-* switch).  Without it a run sets up, warms up, times "
                         "the steps and prints the line")
    return ap.parse_args()


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N child ranks (fresh processes; this parent never touches
    the GPU
    and never exec()s), relay rank 0's output, fail if any rank fails."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    import tempfile
    procs = []
    with tempfile.TemporaryFile() as out0:
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY",
                               "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
        # a rank that dies (an exception in a timed step) must not leave the others waiting in a collective until RCCL's
        # watchdog gives up (round-4 advice): the parent watches all of them and ends the survivors -- its own children,
        # by PID -- as soon as one has failed
        while True:
            rcs = [p.poll() for p in procs]
            if all(rc is not None for rc in rcs):
                break
            if any(rc not in (None, 0) for rc in rcs):
                # (let the failing rank's neighbours fail by themselves first: their messages are the useful ones)
                time.sleep(2.0)
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                rcs = [p.wait() for p in procs]
                break
            time.sleep(0.2)
        out0.seek(0)
        sys.stdout.write(out0.read().decode("utf-8", "replace"))
        sys.stdout.flush()
    if any(rcs):
        raise SystemExit("bench.py: rank exit codes %s" % rcs)


def build_world(args, dev, rank):
    from hybridneuralrendering_amd import scenes
    from hybridneuralrendering_amd.aggregator import PointAggregator
    from hybridneuralrendering_amd.render import HybridRenderer, PointCloud
    sc = scenes.make_scene(args.scene, int(args.points), 2, w=args.width, h=args.height)
    opt = sc.opt
    torch.manual_seed(0)
    agg = PointAggregator(opt)
    with torch.no_grad():          # random-init weights; scale the density head so opacities are spread over (0,1)
        agg.alpha_branch[0].weight.mul_(30.0)
        agg.alpha_branch[0].bias.fill_(30.0)
    agg = agg.to(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cloud = PointCloud(t(sc.xyz), t(sc.emb), t(sc.conf), t(sc.dir), t(sc.color))
    rnd = HybridRenderer(opt, agg, dev)
    # an explicit A/B only: the timed frame runs the library's default otherwise
    if getattr(args, "knn_order", None) and opt.K == 8:
        rnd.knn_order = args.knn_order
    # rank-specific camera: same scene, slightly different pose (weak scaling: every GPU renders a whole frame)
    eye = sc.c2w[:3, 3] + np.array([0.05, -0.04, 0.01], np.float32) * rank
    tgt = sc.c2w[:3, 3] + sc.c2w[:3, 2] * 3.0
    c2w = scenes.look_at(eye, tgt)
    pix = scenes.pixel_grid(sc.w, sc.h, args.margin)
    rays = scenes.camera_rays(pix, sc.intrinsic, c2w)
    cam = dict(raydir=t(rays), campos=t(c2w[:3, 3]), camrot=t(c2w[:3, :3]), bg=t(sc.bg_color),
               c2w_nearest=t(sc.c2w_nearest), campos_nearest=t(sc.c2w_nearest[:, :3, 3]), intrinsic=t(sc.intrinsic),
               images=t(sc.images_nearest), w2c_nearest=torch.inverse(t(sc.c2w_nearest)), c2w=c2w, pix=pix,
               rays_np=rays)
    return sc, opt, agg, cloud, rnd, cam


def render_frame(rnd, cloud, cam, sc, chunk, timers=None, statuses=None):
    R = cam["raydir"].shape[0]
    chunk = R if chunk <= 0 else chunk
    cols = []
    for lo in range(0, R, chunk):
        out = rnd.render_rays(cloud, cam["raydir"][lo:lo + chunk], cam["campos"], cam["camrot"], cam["bg"], sc.near,
                              sc.far,
                              cam["c2w_nearest"], cam["campos_nearest"], cam["intrinsic"], cam["images"],
                              w2c_nearest=cam["w2c_nearest"], timers=timers)
        if statuses is not None and out.get("status") is not None:
            statuses.append(dict(status=out["status"]))
        cols.append(out["coarse_raycolor"])
    return cols[0] if len(cols) == 1 else torch.cat(cols, dim=0), out


def _newest_profile(suffix):
    """profiles/rNN_<suffix> of the latest round that has one (re-collected when kernels change: tools/gpu_job.sh)"""
    for tag in ("r06", "r05", "r04", "r03"):
        if os.path.exists(os.path.join(ROOT, "profiles", "%s_%s" % (tag, suffix))):
            return "%s_%s" % (tag, suffix)
    return "r05_" + suffix


TRAFFIC_JSON = _newest_profile("traffic.json")
TRAIN_TRAFFIC_JSON = _newest_profile("train_traffic.json")
CHAIN_PMC_JSON = _newest_profile("chain_pmc.json")


def pmc_traffic(name=TRAFFIC_JSON):
    """HBM bytes per launch from the rocprofv3 PMC passes kept under profiles/ (FETCH_SIZE / WRITE_SIZE cannot be read
    from inside the process; the passes are re-collected with tools/collect_traffic.py / collect_train_traffic.py
    whenever the kernels change)."""
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", name)))["kernels"]
    except Exception:
        return {}
    return d
