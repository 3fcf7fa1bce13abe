"""The sizing of multi-iteration launches from the per-ray saturation forecast (render_fused.hip, launch_plan.hpp) is scheduling only.  Every output, the per-ray sample hashes and the schedule statistics
are bit-identical with and without it and to one reference iteration per launch; the counters of ngp_render_ctx_schedule_stats show
that they ran.  128 x 128 frames."""
import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu

STATS = ("samples_marched", "samples_slots", "iterations")
ONE_ITER = "one reference iteration per launch"


def _t(x, device):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


class Frames:
    """one scene + model, the rays of a few views, and renders through the fused model with a given flag word"""

    def __init__(self, device, bound, radius, views, H=128, W=128):
        from nerfsafetyvalidation_amd import raymarching
        from nerfsafetyvalidation_amd.scene import StonehengeScene
        self.device, self.W = device, W
        self.sc = StonehengeScene(H=H, W=W, bound=bound, radius=radius)
        self.model = self.sc.build_model(device)
        self.model.fused_cell_table_gb = 0      # no per-cell corner records (copies of table entries, 38 GB): this file is about the schedule
        self.rays = {}
        for v in views:
            self.add_view(v, self.sc)
        self.raymarching = raymarching

    def add_view(self, key, sc, view=None):
        ro, rd = Hh.pinhole_rays(sc.poses[key if view is None else view], sc.intrinsics, sc.H, sc.W)
        self.rays[key] = (_t(ro, self.device), _t(rd, self.device), sc.W)

    def fresh_context(self):
        """the calling thread's render context is destroyed: the next render creates a new one"""
        Hh.fused16(self.model).reset_context()

    def render(self, key, sched, want_last=False):
        """sched: NGP_SCHED_* switches, or ONE_ITER for one reference iteration per launch (a debug flag)
        -> (image, depth, weights_sum, sample hashes), render statistics, schedule counters"""
        from nerfsafetyvalidation_amd import _lib
        flags = _lib.NGP_DBG_ONE_ITER_PER_LAUNCH if sched == ONE_ITER else 0
        o, d, W = self.rays[key]
        fm = Hh.fused16(self.model)
        hashes = torch.zeros(o.shape[0], dtype=torch.int32, device=self.device)
        fm.debug, fm.schedule_flags = (flags, None, hashes), (0 if sched == ONE_ITER else sched)
        try:
            with torch.no_grad():
                nears, fars = self.raymarching.near_far_from_aabb(o, d, self.model.aabb_infer, self.model.min_near)
                ws, depth, image, _, _ = fm.render(self.model, o, d, nears, fars, 0.0, 1024, False, want_last=want_last, frame_width=W)
            sched = fm.schedule_stats()
            torch.cuda.synchronize()
        finally:
            fm.debug, fm.schedule_flags = (0, None, None), 0
        return (image.clone(), depth.clone(), ws.clone(), hashes), dict(fm.last_stats), sched


def assert_same(a, b, what):
    for x, y, name in zip(a[0], b[0], ("image", "depth", "weights_sum", "sample_hash")):
        assert torch.equal(x, y), (what, name)
    for key in STATS:
        assert a[1][key] == b[1][key], (what, key)


@pytest.fixture(scope="module")
def stonehenge(device):
    yield Frames(device, bound=2, radius=1.5, views=(57, 120))
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lego_like(device):
    yield Frames(device, bound=1, radius=3.2, views=(63,))          # test_full_size_frame_properties[lego_configs3] at 128 x 128
    torch.cuda.empty_cache()


def _flag_settings():
    from nerfsafetyvalidation_amd import _lib
    return {"default": 0, "no_forecast": _lib.NGP_SCHED_NO_FORECAST, "one_iter": ONE_ITER}


@pytest.mark.parametrize("setting", ["stonehenge", "lego_like"])
def test_outputs_hashes_and_statistics_are_identical_across_the_switches(setting, request):
    fr = request.getfixturevalue(setting)
    for key in fr.rays:
        outs = {name: fr.render(key, flags) for name, flags in _flag_settings().items()}
        assert (outs["one_iter"][0][3] != 2166136261 - (1 << 32)).float().mean() > 0.1          # not vacuous: many rays marched something (cameras outside the box: 0.3)
        assert outs["one_iter"][1]["replayed"] == 0 and outs["one_iter"][2]["multi_iteration_launches"] == 0
        assert outs["default"][2]["multi_iteration_launches"] > 0
        for name, out in outs.items():
            assert_same(out, outs["one_iter"], (setting, key, name))
            assert out[2]["rolled_back"] == out[1]["replayed"]
        assert outs["no_forecast"][2]["forecast_sized"] == 0


def test_forecast_sizes_launches_and_discards_no_more(stonehenge):
    from nerfsafetyvalidation_amd import _lib
    with_fc = {k: stonehenge.render(k, 0) for k in stonehenge.rays}
    without = {k: stonehenge.render(k, _lib.NGP_SCHED_NO_FORECAST) for k in stonehenge.rays}
    for k in stonehenge.rays:
        print(f"OBS view {k}: discarded samples {with_fc[k][2]['discarded_samples']} (forecast) vs {without[k][2]['discarded_samples']} (death rate alone); "
              f"rolled back {with_fc[k][2]['rolled_back']} vs {without[k][2]['rolled_back']}; launches {with_fc[k][1]['launches']} vs {without[k][1]['launches']}; "
              f"sized by the forecast {with_fc[k][2]['forecast_sized']}")
        assert with_fc[k][2]["forecast_sized"] > 0 and without[k][2]["forecast_sized"] == 0
        assert with_fc[k][2]["discarded_samples"] <= without[k][2]["discarded_samples"]
        assert_same(with_fc[k], without[k], k)


def test_one_context_serves_frames_of_different_sizes(stonehenge):
    """128 x 128, then 32 x 32, then 128 x 128 on one context (forecast on, last-iteration tensors wanted as the renderer
    does by default): each equals the same frame on a fresh context -- no counter of the loop survives from one call into the next."""
    from nerfsafetyvalidation_amd.scene import StonehengeScene
    fr = stonehenge
    if "small" not in fr.rays:
        fr.add_view("small", StonehengeScene(H=32, W=32, bound=2, radius=1.5), view=57)
    fresh = {}
    for key in (57, "small", 120):
        fr.fresh_context()
        fresh[key] = fr.render(key, 0, want_last=True)
    fr.fresh_context()
    for key in (57, "small", 120, "small", 57):
        got = fr.render(key, 0, want_last=True)
        assert_same(got, fresh[key], key)
        for name in ("rolled_back", "discarded_samples", "forecast_sized", "multi_iteration_launches"):
            assert got[2][name] == fresh[key][2][name], (key, name)
