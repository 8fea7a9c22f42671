"""Every size function of the C ABI at the shapes where its layout can go wrong: the boundaries of the 256-byte alignment and the
special cases of each formula (tests/test_scratch_layouts_cpu.py; tools/record_scratch_sizes.py records the table).

`python tests/_scratch_sizes.py all|binning` prints the measured records as one JSON line: gms_binning_bytes depends on GMS_MICRO /
GMS_SEG_LEN, which the library reads once per process, so each environment is measured in a child of its own."""
import itertools
import json
import os
import sys

IMAGE_SHAPES = [(1, 1), (16, 16), (17, 15), (800, 800), (1920, 1080)]
GEOM_P = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 100000]
BINNING_N = [0, 1, 1023, 1024, 1025, 100000, 5000000]
BINNING_SHAPES = [(800, 800), (17, 15)]
# a grid argument is written [n0, n1, n2, voxel] (None: a NULL pointer); 27, 36, 63, 64 and 72 nodes lie either side of the
# boundaries of 8 and of 4 bytes per node
GRIDS = [[3, 3, 3, 0.1], [3, 3, 4, 0.1], [3, 3, 7, 0.1], [4, 4, 4, 0.1], [3, 3, 8, 0.1], [33, 17, 5, 0.5], [64, 64, 64, 0.01], [256, 256, 256, 0.01]]
BAD_GRIDS = [[2, 8, 8, 0.1], [8, 8, 8, 0.0], None]


def cases(which="all"):
    """[(function name, [arguments])]"""
    out = [("gms_binning_bytes", [n, w, h]) for (w, h) in BINNING_SHAPES for n in BINNING_N + [-1]]
    if which == "binning":
        return out
    out += [("gms_geom_bytes", [p]) for p in GEOM_P + [-1]]
    for fn in ("gms_image_bytes", "gms_image_n_contrib_offset", "gms_image_counts_offset"):
        out += [(fn, [w, h]) for (w, h) in IMAGE_SHAPES]
    # N * 16 and N * 4 cross 256 at 16 and 64; the cell tables ((N / 2 + 65) * 4) at every 128 points; grid_max_cells caps above 8 M
    out += [("gms_knn_workspace_bytes", [n]) for n in (-1, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000, 100000, 9000000)]
    # 12 bytes per centroid cross 256 between 21 and 22 (and 64 is a multiple again)
    sizes = (0, 1, 21, 22, 63, 64, 65, 100000)
    out += [("gms_bind_workspace_bytes", [p, f]) for p, f in itertools.product(sizes, sizes)]
    out += [("gms_bind_workspace_bytes", [-1, -1])]
    out += [("gms_density_grid_workspace_bytes", [g, p]) for g in GRIDS for p in (0, 1, 63, 64, 65, 100000)]
    out += [("gms_density_grid_workspace_bytes", [g, 64]) for g in BAD_GRIDS] + [("gms_density_grid_workspace_bytes", [GRIDS[0], -1])]
    out += [("gms_grid_components_workspace_bytes", [g]) for g in GRIDS + BAD_GRIDS]
    out += [("gms_l1_ssim_partials", list(a)) for a in ((0, 16, 16), (1, 1, 1), (3, 16, 16), (3, 17, 15), (3, 800, 800), (-1, 16, 16), (3, 0, 0))]
    out += [("gms_flame_workspace_bytes", list(a)) for a in ((0, 5, 0), (1, 5, 1), (63, 5, 100), (64, 5, 100), (65, 5, 100), (5023, 5, 400),
                                                             (5023, 2, 0), (-1, 1, -1), (100000, 16, 150))]
    # one flag byte per Gaussian; 12 bytes per block of 256 cross 256 between 21 and 22 blocks
    out += [("gms_densify_plan_workspace_bytes", [p]) for p in (-1, 0, 1, 255, 256, 257, 5376, 5377, 5632, 5633, 100000, 1 << 30)]
    out += [("gms_image_metrics_workspace_bytes", list(a)) for a in ((0, 3, 8, 8), (1, 3, 1, 1), (1, 3, 16, 16), (1, 3, 17, 15), (4, 3, 800, 800),
                                                                     (2, 4, 63, 65), (-1, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8))]
    out += [("gms_lpips_workspace_bytes", list(a)) for a in ((0, 64, 64), (-1, 64, 64), (1, 0, 64), (1, 64, -1), (1, 16, 16), (1, 17, 15),
                                                             (1, 64, 64), (2, 65, 63), (3, 255, 257), (4, 256, 256), (8, 800, 800))]
    out += [("gms_ground_truth_workspace_bytes", list(a)) for a in ((0, 800, 800, 400, 400), (1, 1, 1, 1, 1), (1, 800, 800, 400, 400),
                                                                    (2, 800, 800, 800, 800), (3, 17, 15, 8, 7), (1, 17, 15, 17, 7))]
    out += [("gms_resize_workspace_bytes", list(a)) for a in ((0, 100, 100, 3, 50, 50), (1, 1, 1, 4, 1, 1), (1, 100, 100, 3, 50, 50),
                                                              (1, 100, 100, 3, 100, 50), (1, 100, 100, 3, 50, 100), (2, 17, 15, 4, 8, 7),
                                                              (1, 4946, 3286, 3, 1600, 1063))]
    return out


def measure(which="all"):
    """[[function name, [arguments], value]] from the library this process loads"""
    from diff_gaussian_rasterization import _lib
    lib = _lib.load()

    def arg(a):
        if isinstance(a, list):
            return _lib.GridSpec((_lib.C.c_int32 * 3)(*a[:3]), (_lib.C.c_float * 3)(0.0, 0.0, 0.0), a[3])
        return a

    return [[fn, args, int(getattr(lib, fn)(*[arg(a) for a in args]))] for fn, args in cases(which)]


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "gaussian-mesh-splatting_amd"))
    print(json.dumps(measure(sys.argv[1] if len(sys.argv) > 1 else "all")))
