"""draw() with colliders in the picture (egg_set_collider_styles, DESIGN.md section 2.7 "Collider styles"): ms per draw(),
wall clock around the call with rgba = NULL (the image stays on the device; the call ends with the render stream idle), after
a warm-up.  One JSON line per mode.  The scene is BASELINE config 2 as profiles/r02_render_cfg2.md draws it: 256 batches,
3 steps, both canvases at the 2560 px cap, a 2640 x 2640 px screen.

    python scripts/gpu_collider_draw_bench.py [--draws 40] [--warmup 5] [--modes unset,1,8,64] [--package-root DIR] [--label TEXT]

modes: unset = no style is ever set (the only mode an earlier commit has); N = a list of N colliders, all visible, measured
twice in the same process: unstyled (`ms_unstyled`) and styled (`ms_styled`); `culled_tile_share` is the share of the
screen's 16 x 16 px tiles the kernel's cull rule gives an empty mask, evaluated here in numpy over the tile centres.
--package-root imports the package from another checkout (a build of an earlier commit: mode unset only), so that two
builds can be compared in one session, alternating.  Run one mode per process for a figure that is to be relied on.  The
kernels' own times come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/... --modes 64):
egg_render_colliders_kernel beside egg_render_composite_kernel in the same run."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import grid_positions  # noqa: E402

TILE = 16


def colliders_of(n, lo_x, lo_y, size):
    """n colliders over a size x size px view at (lo_x, lo_y), all visible: a floor, a ring round the scene, discs, walls"""
    rng = np.random.default_rng(25)
    mid_x, mid_y = lo_x + 0.5 * size, lo_y + 0.5 * size
    out = [(("half_plane", 0.0, -1.0, -(lo_y + size - 90.0)), {"fill": (0.3, 0.25, 0.2, 1.0), "line": (1, 1, 1, 1), "line_width": 2.0})]
    if n > 1:
        out.append((("container", mid_x, mid_y, 0.5 * size - 30.0), {"line": (0.6, 0.6, 0.7, 0.8), "line_width": 3.0}))
    while len(out) < min(n, 8):
        x, y = lo_x + size * rng.uniform(0.1, 0.9, 2)
        out.append((("disc", float(x), float(y), float(rng.uniform(20.0, 120.0))), {"fill": (0.1, 0.5, 0.8, 0.6), "line": (1, 1, 1, 1), "line_width": 1.5,
                                                                                 "layer": "over"}))
    while len(out) < n:
        x, y = lo_x + size * rng.uniform(0.05, 0.95, 2)
        a, l = rng.uniform(0.0, np.pi), rng.uniform(100.0, 900.0)
        out.append((("wall", float(x), float(y), float(x + l * np.cos(a)), float(y + l * np.sin(a))), {"line": (0.9, 0.8, 0.3, 1.0), "line_width": 2.0}))
    return [c for c, _ in out[:n]], [s for _, s in out[:n]]


def culled_share(colliders, styles, origin, size):
    """the kernel's cull rule (csrc/eggsim_render.hip) at every tile centre, per layer: the share of (tile, launch) pairs
    whose mask is empty"""
    import collider_draw_model as cdm
    tiles = (size + TILE - 1) // TILE
    cx = ((np.arange(tiles) * TILE + 0.5 * TILE) + origin[0])[None, :]
    cy = ((np.arange(tiles) * TILE + 0.5 * TILE) + origin[1])[:, None]
    shares = []
    for layer in (0, 1):
        reach = np.zeros((tiles, tiles), bool)
        any_visible = False
        for c, s in zip(colliders, styles):
            st = cdm.style_of(s)
            if not cdm.visible(c, s) or st["layer"] != layer:
                continue
            any_visible = True
            p = np.abs(np.array(cdm._params(c)))
            sd = cdm.signed_distance(c, cx, cy) + np.zeros((tiles, tiles))
            half = 0.5 * (TILE - 1)
            spread = ((p[0] + p[1]) * half if c[0] == "half_plane" else 1.4142135623730951 * half) + 1.0 + (np.abs(cx) + np.abs(cy) + p.sum()) * 2.0 ** -40
            fills = cdm.INSIDE[c[0]] and st["fill"][3] > 0
            lines = st["line"][3] > 0 and st["line_width"] > 0
            if fills:
                reach |= ~(sd - spread >= 0.5)
            if lines:
                reach |= ~(np.abs(sd) - spread >= 0.5 + 0.5 * float(st["line_width"]))
        if any_visible:
            shares.append(1.0 - reach.mean())
    return shares


def run(mode, draws, warmup):
    from egg_fluid_simulation_amd import SimulationHandler
    xs, ys, _ = grid_positions(256)
    h = SimulationHandler()
    h.add_many(xs, ys, 50, 15)
    for _ in range(3):
        h.step(1 / 60, 2, 3)
    lo_x, lo_y = float(xs.min() - 120.0), float(ys.min() - 120.0)
    size = int(xs.max() + 120.0 - lo_x)
    p = h._render_params((size, size), (lo_x, lo_y), None, (0.0, 0.0, 0.0, 0.0), None, True)
    render = h._c("render")

    def timed():
        for _ in range(warmup):
            assert render(C.byref(p), None) == 0
        s0 = h.stats()["kernel_launches"]
        samples = []
        for _ in range(draws):
            t0 = time.perf_counter()
            assert render(C.byref(p), None) == 0
            samples.append(1e3 * (time.perf_counter() - t0))
        return dict(mean=float(np.mean(samples)), median=float(np.median(samples)), min=float(np.min(samples)), max=float(np.max(samples)),
                    launches_per_draw=(h.stats()["kernel_launches"] - s0) / draws)

    n_w, n_y = h.get_n_particles()
    out = {"scene": "config2", "mode": mode, "particles": n_w + n_y, "screen": size, "draws": draws, "warmup": warmup}
    if mode == "unset":
        out["ms_unstyled"] = timed()
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        colliders, styles = colliders_of(int(mode), lo_x, lo_y, size)
        h.set_solver_order("relaxed")  # (a list needs relaxed order; draw() does not care)
        h.set_colliders(colliders)
        out["ms_unstyled"] = timed()
        h.set_collider_styles(styles)
        out["ms_styled"] = timed()
        out["ms_added_median"] = out["ms_styled"]["median"] - out["ms_unstyled"]["median"]
        out["culled_tile_share_per_launch"] = culled_share(h.get_colliders(), styles, (lo_x, lo_y), size)
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="unset,1,8,64")
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.package_root:
        sys.path.insert(0, os.path.abspath(a.package_root))
    for mode in a.modes.split(","):
        print(json.dumps(dict(run(mode, a.draws, a.warmup), label=a.label)), flush=True)


if __name__ == "__main__":
    main()
