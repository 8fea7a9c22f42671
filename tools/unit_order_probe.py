"""What a unit order does to `micro_bwd` ON THE CHIP, without a kernel for it: between a frame's forward and its backward the present units'
32-byte records of the unit table are permuted in place (the kept binning buffer is the one the backward reads; `micro_bwd` takes everything
it knows of a unit from that record, so it computes the same sums in another block order), and the launch's span is read from the phase
stamps.  The companion of the offline replay `tools/unit_order_study.py bwd`, which can only assume that a block takes as long wherever it runs.

Needs the EXPERIMENTS build (tools/build_experiments.sh); run on the GPU box:

    LD_LIBRARY_PATH=gaussian-mesh-splatting_amd/lib_exp GMSPLAT_LIB=gaussian-mesh-splatting_amd/lib_exp/libgmsplat.so GMS_DBG=1024 \
        python tools/unit_order_probe.py [workload] [repetitions]

Orders: the table's own; the length of the unit's longest 4x4-block list (what unit_stage's S.ocnt[0] holds) as a stable partition into
K = 8 / 16 / 32 classes, table order inside a class; the entries the block's longest wave walked and the block's measured duration, both
taken from an EARLIER repetition in table order (more than any key known before the launch could say).  The arms alternate.
"""
import ctypes as C, os, sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def unit_costs(dgr, lib, torch, W, H):
    """Per unit of the last frame's unit table: the length of its longest 4x4-block list, counted from the block masks the forward left
    (what unit_stage's S.ocnt[0] holds), whether the unit has entries, and the table itself as a [units, 8] int32 VIEW of the kept binning
    buffer.  Needs keep_buffers(True) before the frame."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _staircase as S
    st, raw = dgr.last_stats(), dgr.raw_buffers()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    N, hint = int(st["num_rendered"]), int(st["capacity_hint"])
    cap = hint if hint > 0 and hint >= N else N
    L_carve = min(int(os.environ.get("GMS_SEG_LEN", 256)), 256)
    ba, bbytes = S.binning_layout(cap, T, L_carve, True)
    assert bbytes == int(lib.gms_binning_bytes(cap, W, H)) and raw["binning"].numel() >= bbytes, (cap, bbytes)
    tabs = S.read_tables(raw["image"], raw["binning"], W, H, cap, L_carve, True)
    L, units = int(tabs["scan_out"][3]), tabs["units"].astype(np.int64)
    mm = raw["binning"][ba["mmask"]:ba["mmask"] + 2 * N].view(torch.int16).cpu().numpy().view(np.uint16)
    beg = units[:, 4] + units[:, 1] * L
    end = np.minimum(units[:, 5], beg + L)
    bits = ((mm[:, None] >> np.arange(16)[None, :]) & 1).astype(np.int64)
    csum = np.concatenate([np.zeros((1, 16), np.int64), np.cumsum(bits, axis=0)])
    cost = (csum[np.maximum(end, beg)] - csum[beg]).max(axis=1)
    # (.data: a write through this view is not counted against the tensor the frame's backward saved)
    table = raw["binning"].data[ba["units"]:ba["units"] + 32 * len(units)].view(torch.int32).view(-1, 8)
    return cost, end > beg, table


def main():
    os.environ.setdefault("GMS_DBG", "1024")
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gaussian-mesh-splatting_amd"))
    import torch
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _lib
    from games_hip import synthetic as syn
    from games_hip.model import HipGaussianMeshModel
    from games_hip.render import PipelineParams, render

    wl = sys.argv[1] if len(sys.argv) > 1 else "c2_hotdog_like"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    scene = syn.mesh_scene(wl, state="trained")
    size = scene.meta["image"]
    model = HipGaussianMeshModel.from_scene(scene, "cuda")
    cam = syn.orbit_camera(0, width=size, height=size).to("cuda"); bg = torch.ones(3, device="cuda")
    lib = _lib.load()
    lib.gms_debug_read.argtypes = [C.c_void_p, C.c_size_t]
    dgr.keep_buffers(True)
    buf = np.zeros(4 * 65536 * 8, np.uint64)

    def step(order_of):
        """one forward + backward; order_of(cost, present) -> present units by rank, or None for the table's order.
        -> (span of micro_bwd in us, per-unit block duration, per-unit entries walked, cost, present, gradient checksum)"""
        model.update_alpha(); model.prepare_scaling_rot()
        img = render(cam, model, PipelineParams(), bg)["render"]
        cost, present, table = unit_costs(dgr, lib, torch, size, size)
        npres = int(present.sum())
        assert present[:npres].all(), "the present units are expected in front of the empty tiles' units"
        order = None if order_of is None else order_of(cost, present)
        if order is not None:
            assert len(order) == npres and np.array_equal(np.sort(order), np.arange(npres)), "not a permutation of the present units"
            table[:npres] = table[torch.from_numpy(order).to(table.device)]
        img.backward((img.detach() - 0.5) / img.numel())
        check = sum(float(p.grad.double().abs().sum()) for p in model.parameters() if p.grad is not None)
        for p in model.parameters(): p.grad = None
        torch.cuda.synchronize()
        if lib.gms_debug_read(buf.ctypes.data_as(C.c_void_p), buf.nbytes) != 0:
            sys.exit("no stamps: not an EXPERIMENTS build, or GMS_DBG & 1024 unset")
        b = buf.reshape(4, 65536, 8).astype(np.int64)
        live = (b[:, :, 0] > 0) & (b[:, :, 5] > 0)
        blk = np.nonzero(live.all(axis=0))[0]
        start, end = b[:, blk, 0].min(axis=0), b[:, blk, 5].max(axis=0)
        rank = (b[0, blk, 7] >> 40) & 0xffffff                    # the index the block loaded its record from
        unit = rank if order is None else order[rank]
        udur, utrips = np.zeros(len(cost)), np.zeros(len(cost))
        udur[unit] = (end - start) / 100.0
        utrips[unit] = b[:, blk, 6].max(axis=0)
        return (end.max() - start.min()) / 100.0, udur, utrips, cost, present, check

    for _ in range(3):
        span0, udur0, utrips0, cost0, present0, check0 = step(None)

    def classes(K):
        def f(cost, present):
            idx = np.nonzero(present)[0]
            return idx[np.argsort((K - 1 - np.minimum(K - 1, cost * K // 257))[idx], kind="stable")]
        return f

    def descending(key):
        return lambda cost, present: np.nonzero(present)[0][np.argsort(-key[present], kind="stable")]

    arms = {"table order": None, "key, K = 8": classes(8), "key, K = 16": classes(16), "key, K = 32": classes(32),
            "entries walked (earlier repetition), descending": descending(utrips0),
            "measured duration (earlier repetition), descending": descending(udur0)}
    spans, checks = {n: [] for n in arms}, {n: [] for n in arms}
    for r in range(reps):
        names = list(arms) if r % 2 == 0 else list(arms)[::-1]
        for n in names:
            s, _, _, cost, present, chk = step(arms[n])
            assert np.array_equal(cost, cost0) and np.array_equal(present, present0), "the frame changed between repetitions"
            spans[n].append(s); checks[n].append(chk)
    print(f"workload {wl}: micro_bwd span by the phase stamps, {reps} repetitions per order, orders alternating (us: min / median / max)")
    for n, v in spans.items():
        print(f"  {n:52s}: {min(v):6.1f} / {np.median(v):6.1f} / {max(v):6.1f}   sum |grad| relative to the table order's: "
              f"{np.mean(checks[n]) / np.mean(checks['table order']) - 1:+.1e}")


if __name__ == "__main__":
    main()
