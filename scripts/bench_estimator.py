#!/usr/bin/env python3
"""The state estimator's cost (nav/estimator.py, nav/features.py): the keypoint detector at 800 x 800 (HIP against the numpy
restatement), one estimate_state at 800 x 800 (1024 pixels, 512 samples, 100 iterations) split into detection, Adam loop and
Hessian, and a 64 x 64 rollout step with and without the estimator (blob sensor frames, so that every step runs the fit).  Appends JSON lines to profiles/estimator_bench.jsonl."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from nerfsafetyvalidation_amd import rollout as RO
from nerfsafetyvalidation_amd import scene as SC
from nerfsafetyvalidation_amd.nav import features as FE, sift_numpy as S
from nerfsafetyvalidation_amd.nav.estimator import Estimator, estimator_config
from nerfsafetyvalidation_amd.nerf.utils import get_rays
from nerfsafetyvalidation_amd.scene import StonehengeScene

dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "estimator_bench.jsonl")
lines = []


def emit(d):
    print(json.dumps(d), flush=True)
    lines.append(d)


H = W = 800
sc = StonehengeScene(H=H, W=W, bound=2)
model = sc.build_model(dev, backbone="linear", cuda_ray=False, fp16_table=False)
model.requires_grad_(False)
kw = dict(staged=True, bg_color=1.0, perturb=False, num_steps=512, upsample_steps=0)
rays = get_rays(torch.from_numpy(sc.poses[7:8]).float().to(dev), sc.intrinsics, H, W)
with torch.no_grad():
    img = torch.squeeze(model.render(rays["rays_o"], rays["rays_d"], **kw)["image"]).float().cpu().numpy().reshape(H, W, 3)
img = (img * 255).astype(np.uint8)
blobs = S.blob_frame(H, W, 0)              # (the synthetic scene's smooth renders hold few keypoints; the fit below needs some)
frame = torch.from_numpy(img).to(dev)
for _ in range(3):
    FE.sift_interest_mask(frame)
torch.cuda.synchronize()
n = 20
t0 = time.perf_counter()
for _ in range(n):
    out = FE.sift_interest_mask(frame)
torch.cuda.synchronize()
hip_ms = (time.perf_counter() - t0) / n * 1e3
t0 = time.perf_counter()
S.interest_mask(img)
np_ms = (time.perf_counter() - t0) * 1e3
emit({"what": "detector 800x800 (keypoints + dilated mask)", "hip_ms": round(hip_ms, 3), "numpy_ms": round(np_ms, 1),
      "keypoints": int(out["count"].item())})


class Agent:
    @staticmethod
    def drone_dynamics(x, action):
        return RO.drone_dynamics(x, action, 2.0 / 12)


class Timed(Estimator):
    def interest_regions(self, image):
        torch.cuda.synchronize(); t = time.perf_counter()
        r = super().interest_regions(image)
        self.t_detect = (time.perf_counter() - t) * 1e3
        return r

    def measurement_hessian(self, state, sig):
        torch.cuda.synchronize(); t = time.perf_counter()
        h = super().measurement_hessian(state, sig)
        torch.cuda.synchronize()
        self.t_hess = (time.perf_counter() - t) * 1e3
        return h


pose = torch.from_numpy(sc.poses[7]).float()
state = torch.zeros(12)
state[:3] = torch.linalg.solve(torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), pose[:3, 3])
for rep in range(2):
    e = Timed(estimator_config(dev), Agent(), state.clone(), seed=0,
              get_rays_fn=lambda p, inds: get_rays(p.to(dev), sc.intrinsics, H, W, inds=inds), render_fn=lambda o, d: model.render(o, d, **kw))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    e.estimate_state(blobs, None, torch.tensor([10.0, 0.0, 0.0, 0.0]))
    torch.cuda.synchronize(); total = (time.perf_counter() - t0) * 1e3
if e.success:
    emit({"what": "estimate_state 800x800, 1024 px, 512 samples, 100 iterations (eager, fp32)", "total_ms": round(total, 1),
          "detect_ms": round(e.t_detect, 2), "hessian_ms": round(e.t_hess, 2),
          "adam_loop_ms": round(total - e.t_detect - e.t_hess, 1), "keypoints": e.keypoints, "loss_first_last": [e.losses[0], e.losses[-1]]})
else:
    emit({"what": "estimate_state 800x800", "success": False, "total_ms": round(total, 1)})

# rollout step, 64 x 64, with the planner, with and without the estimator.  The map is the planner fixture's (one A* can plan
# through); its frames hold no keypoint, so the estimator's sensor image is a blob frame instead -- every step then runs the full fit
def planner_net():
    from nerfsafetyvalidation_amd.nerf.network import NeRFNetwork
    f = np.load(os.path.join(ROOT, "tests", "golden", "planner.npz"))
    net = NeRFNetwork(encoding="hashgrid", bound=int(f["bound"]), cuda_ray=False, density_scale=1, min_near=0.2, density_thresh=0.01, bg_radius=-1)
    g = torch.Generator().manual_seed(int(f["table_seed"]))
    net.encoder.embeddings.data.copy_(torch.rand(net.encoder.embeddings.shape, generator=g) - 0.5)
    for i, l in enumerate(net.sigma_net):
        l.weight.data.copy_(torch.from_numpy(f[f"sigma{i}"]))
    for i, l in enumerate(net.color_net):
        l.weight.data.copy_(torch.from_numpy(f[f"color{i}"]))
    return net.to(dev).eval().requires_grad_(False)


flags = []


class BlobSensor(RO.RolloutSimulator):
    def observe(self, pose):
        sigma = super().observe(pose)
        if self.estimator is not None:
            self.sensor_image = S.blob_frame(self.H, self.W, len(self.poses))
        return sigma

    def estimate(self, k, state):
        est = super().estimate(k, state)
        flags.append((bool(self.estimator.success), self.estimator.keypoints))
        return est


net = planner_net()
h = w = 64
rk = dict(num_steps=64, upsample_steps=0, max_ray_batch=4096)
pcfg = RO.planner_config(dev, epochs_update=250)
RO.RolloutSimulator, keep = BlobSensor, RO.RolloutSimulator
for name, ecfg in (("planner", None), ("planner + estimator (blob sensor frames)", estimator_config(dev))):
    RO.run_rollout(net, SC.intrinsics(h, w), h, w, 1, 2, seed=1, in_flight=1, render_kwargs=rk, autocast=False, planner_cfg=pcfg, estimator_cfg=ecfg)
    flags.clear()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    rows, c = RO.run_rollout(net, SC.intrinsics(h, w), h, w, 1, 4, seed=1, in_flight=1, render_kwargs=rk, autocast=False, planner_cfg=pcfg,
                             estimator_cfg=ecfg)
    torch.cuda.synchronize()
    d = {"what": f"rollout step 64x64, {name}", "ms_per_step": round((time.perf_counter() - t0) * 1e3 / c["steps"], 1), "steps": c["steps"]}
    if ecfg is not None:
        d["estimator_success"] = [f for f, _ in flags]
        d["keypoints"] = [n for _, n in flags]
    emit(d)
RO.RolloutSimulator = keep

with open(OUT, "a") as f:
    for d in lines:
        f.write(json.dumps(d) + "\n")
