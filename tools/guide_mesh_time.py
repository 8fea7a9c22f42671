#!/usr/bin/env python3
"""Time the guide-mesh estimate (csrc/guide_mesh.hip) on games_hip.synthetic's flat scene: device events, median of 20 runs.

    python tools/guide_mesh_time.py [--P 498800 997600] [--resolution 128 256] [--level 0.5] [--runs 20] [--scipy] [--json out.json]

Per (P, resolution): the field (bounds given: launches only), the extraction (flag, scan, the counts' read-back, emit), the whole
estimate from the Gaussians to the mesh by the wall clock with both host waits in it, V and F, and the rate of the 64-bit atomics in
added bytes per second (8 bytes per add; MI355X_MICROARCH.md gives 1.3 TB/s for float atomics of 4 bytes).  The number of adds is the
expected number of nodes inside the 3-sigma ellipsoids, sum of their volumes / voxel volume: exact in expectation for centres that are
uniform relative to the lattice, as this scene's are; the nodes of the boxes, which the lanes visit, are counted exactly.

Also the components of the grid (csrc/grid_components.hip): labels and sizes, the cleaning (fill_cavities with min_component_nodes = 200:
two labelling passes, the sizes, the two rewrites), the extraction from the cleaned grid with its V and F, and the numbers of inside
components and cavities.  With --scipy, scipy.ndimage.label of the inside nodes on the CPU for the same grid, as context only."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))

import torch  # noqa: E402

from games_hip import guide_mesh as gm, synthetic as syn  # noqa: E402


def event_ms(fn, runs):
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def box_and_ellipsoid_nodes(means, scales, rotations, grid, min_sigma_voxels=1.0):
    """(nodes of the clipped boxes, expected nodes inside the ellipsoids) -- the kernel's box statements in torch"""
    h = grid.voxel
    sigma = scales.clamp_min(min_sigma_voxels * h)
    r, x, y, z = rotations.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    ext = gm.CUTOFF * ((R * sigma[:, None, :]) ** 2).sum(-1).sqrt()
    org = torch.tensor(grid.origin, device=means.device)
    n = torch.tensor(grid.n, device=means.device, dtype=torch.float32)
    lo = torch.floor((means - ext - org) / h).clamp_min(0)
    hi = torch.minimum(torch.ceil((means + ext - org) / h), n - 1)
    box = (hi - lo + 1).clamp_min(0).double().prod(1)
    ell = 4.0 / 3.0 * math.pi * gm.CUTOFF ** 3 * sigma.double().prod(1) / h ** 3
    return float(box.sum()), float(ell.sum()), int((box > 16384).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[498800, 997600])
    ap.add_argument("--resolution", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--level", type=float, default=0.5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--min-component-nodes", type=int, default=200)
    ap.add_argument("--scipy", action="store_true", help="also time scipy.ndimage.label on the CPU (context only)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for P in a.P:
        sc = syn.flat_scene(P).to("cuda")
        m, s, q, o = sc.means3D.contiguous(), sc.scales.contiguous(), sc.rotations.contiguous(), sc.opacities.reshape(-1).contiguous()
        for res in a.resolution:
            g = gm.density_grid(m, s, q, o, resolution=res)                          # (warm-up; its box is the bounds of the timed runs)
            bounds = (g.origin, tuple(g.origin[k] + (g.n[k] - 1) * g.voxel for k in range(3)))
            box, ell, big = box_and_ellipsoid_nodes(m, s, q, g)
            v, f = gm.surface_nets(g, a.level)
            field = event_ms(lambda: gm.density_grid(m, s, q, o, resolution=max(g.n), bounds=bounds), a.runs)
            extract = event_ms(lambda: gm.surface_nets(g, a.level), a.runs)
            label = event_ms(lambda: gm.grid_components(g, a.level), a.runs)
            clean = event_ms(lambda: gm.clean_grid(g, a.level, fill_cavities=True, min_component_nodes=a.min_component_nodes), a.runs)
            gc = gm.clean_grid(g, a.level, fill_cavities=True, min_component_nodes=a.min_component_nodes)
            vc, fc = gm.surface_nets(gc, a.level)
            extract_clean = event_ms(lambda: gm.surface_nets(gc, a.level), a.runs)
            labels, sizes = gm.grid_components(g, a.level)
            roots = sizes.reshape(-1).nonzero().reshape(-1)
            root_inside = (g.values.reshape(-1)[roots] >= a.level) & (roots != 0)
            scipy_ms = None
            if a.scipy:
                from scipy import ndimage
                inside = (g.values >= a.level).cpu().numpy()
                t0 = time.perf_counter()
                ndimage.label(inside)
                scipy_ms = (time.perf_counter() - t0) * 1e3
            wall = []
            for _ in range(a.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gm.surface_nets(gm.density_grid(m, s, q, o, resolution=res), a.level)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
            row = dict(P=P, resolution=res, n=g.n, voxel=g.voxel, level=a.level, V=int(v.shape[0]), F=int(f.shape[0]), field_ms=field[0], field_min_ms=field[1],
                       extract_ms=extract[0], extract_min_ms=extract[1], total_wall_ms=statistics.median(wall), box_nodes=box, expected_adds=ell,
                       label_ms=label[0], label_min_ms=label[1], clean_ms=clean[0], clean_min_ms=clean[1], extract_clean_ms=extract_clean[0],
                       extract_clean_min_ms=extract_clean[1], V_clean=int(vc.shape[0]), F_clean=int(fc.shape[0]), inside_components=int(root_inside.sum()),
                       cavities=int((~root_inside).sum()) - 1, min_component_nodes=a.min_component_nodes, scipy_label_cpu_ms=scipy_ms, list_gaussians=big, atomic_added_TB_per_s=8 * ell / (field[0] * 1e-3) / 1e12, field_max=float(g.values.max()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
