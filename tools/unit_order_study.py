"""Offline: what a better block order would buy the micro-tile forward launches (round 6).  Input: the per-block records tools/micro_fwd_phases.py
dumps with GMS_PHASES_DUMP (start / staged / end of every block, its unit's kind, segment, entries, its tile's list length).  The launch is
replayed as greedy list scheduling on `slots` block slots (the dispatcher starts the next block of the grid whenever a slot frees) with the
measured block durations, under: the grid's own order, longest-first (the ideal a static order can reach), and candidate keys that are
known when the unit table is written (the tile's list length, the segment index).

    python tools/unit_order_study.py bwd run1.npz run2.npz ...

replays the micro-tile BACKWARD instead, from the dumps tools/micro_phases.py writes with GMS_DBG=1024 GMS_PHASES_DUMP=...: 1 280 block
slots (five blocks per CU), the grid's order, longest-first by the run's own durations (hindsight) and by another run's (what is left of
that without the run's own noise), the exact number of entries the block's longest wave walked, and the key the forward could leave
behind -- the length of the unit's longest 4x4-block list -- as a stable partition into K classes, table order inside a class.  An order is a list of units by RANK; the
launch deals ranks to blocks the way load_unit_at does (runs of `unit_run` ranks per XCD), and the replay starts blocks in block order."""
import heapq
import sys

import numpy as np


def makespan(dur, order, slots):
    h = [0.0] * slots
    heapq.heapify(h)
    end = 0.0
    for i in order:
        t = heapq.heappop(h) + dur[i]
        end = max(end, t)
        heapq.heappush(h, t)
    return end


def class_order(cost, present, K):
    """units by rank: classes of descending cost, table order inside a class, absent units left out"""
    cls = K - 1 - np.minimum(K - 1, cost * K // 257)
    idx = np.nonzero(present)[0]
    return idx[np.argsort(cls[idx], kind="stable")]


def dispatch(order, run):
    """order (units by rank) -> units in the order their blocks start: block b takes rank ((s / run) * 8 + xcd) * run + s % run, s = b >> 3"""
    n = len(order)
    nb = 8 * run * ((n + 8 * run - 1) // (8 * run))
    b = np.arange(nb)
    s, xcd = b >> 3, b & 7
    rank = ((s // run) * 8 + xcd) * run + s % run
    return order[rank[rank < n]]


def bwd_study(paths, slots=1280):
    runs = []
    for path in paths:
        z = np.load(path)
        unit, dur = z["unit"].astype(np.int64), z["end"] - z["start"]
        cost = z["unit_cost"].astype(np.int64)
        udur, utrips = np.zeros(len(cost)), np.zeros(len(cost))
        udur[unit], utrips[unit] = dur, z["trips"]          # (units without stamps returned at once: 0)
        runs.append(dict(path=path, z=z, unit=unit, dur=dur, cost=cost, present=z["unit_present"], run=int(z["unit_run"]), udur=udur, utrips=utrips))
    spans = {}
    for k, r in enumerate(runs):
        z, unit, dur, cost, present, run, udur = r["z"], r["unit"], r["dur"], r["cost"], r["present"], r["run"], r["udur"]
        print(f"{r['path']}: {len(unit)} stamped blocks of {int(present.sum())} present units ({len(cost)} in the table), measured span {z['end'].max():.1f} us, "
              f"sum of durations {dur.sum():.0f} block-us = {dur.sum() / slots:.1f} us on {slots} slots, longest block {dur.max():.1f} us")
        print(f"  key (longest block list) against measured block duration: corr {np.corrcoef(cost[unit], dur)[0, 1]:+.3f}; "
              f"against the block's entries walked {np.corrcoef(cost[unit], z['trips'])[0, 1]:+.3f}; entries walked against duration "
              f"{np.corrcoef(z['trips'], dur)[0, 1]:+.3f}; start time against duration {np.corrcoef(z['start'], dur)[0, 1]:+.3f}")
        descending = lambda key: np.argsort(-key, kind="stable")
        res = {"grid order": makespan(udur, dispatch(np.arange(len(cost)), run), slots),
               "longest first, own durations (hindsight)": makespan(udur, dispatch(descending(udur), run), slots)}
        # the same unit's duration in ANOTHER run is the best any key could know: what is left of the hindsight figure without this run's noise
        for j, o in enumerate(runs):
            if j != k and len(o["udur"]) == len(udur):
                res[f"longest first, durations of run {j + 1}"] = makespan(udur, dispatch(descending(o["udur"]), run), slots)
                m = (udur > 0) & (o["udur"] > 0)
                print(f"  the same unit in run {j + 1}: corr {np.corrcoef(udur[m], o['udur'][m])[0, 1]:+.3f}, mean |difference| {np.abs(udur[m] - o['udur'][m]).mean():.1f} us")
        res["entries walked (exact), descending"] = makespan(udur, dispatch(descending(r["utrips"]), run), slots)
        for K in (8, 16, 32):
            res[f"key, K = {K}"] = makespan(udur, dispatch(class_order(cost, present, K), run), slots)
        for name, v in res.items():
            print(f"  replay, {name:42s}: {v:6.1f} us")
            spans.setdefault(name.replace(f"of run {2 - k}", "of the other run") if len(runs) == 2 else name, []).append(v)
    if len(paths) > 1:
        print("over the runs (min .. max):")
        for name, v in spans.items():
            print(f"  {name:42s}: {min(v):6.1f} .. {max(v):6.1f} us")


if len(sys.argv) > 1 and sys.argv[1] == "bwd":
    bwd_study(sys.argv[2:])
    sys.exit(0)

for path in sys.argv[1:]:
    z = np.load(path)
    dur = z["end"] - z["start"]
    walk = z["end"] - z["staged"]
    n = len(dur)
    order0 = np.argsort(z["block"])
    slots = 2048
    print(f"{path}: {n} blocks, measured span {z['end'].max():.1f} us, sum of durations {dur.sum():.0f} block-us = {dur.sum() / slots:.1f} us on {slots} slots, longest block {dur.max():.1f}")
    print(f"  replay, grid order            : {makespan(dur, order0, slots):5.1f} us")
    print(f"  replay, longest first (ideal) : {makespan(dur, np.argsort(-dur), slots):5.1f} us")
    te, seg, nseg, ent, kind = z["tile_entries"].astype(float), z["seg"], z["nseg"], z["entries"], z["kind"]
    keys = {
        "shallow tiles first (ascending tile list length among non-empty)": np.where(ent > 0, te, 1e12),
        "first segments of shallow tiles, then by segment index descending": np.where(ent > 0, te * 1e-3 - (seg == 0) * 1e6 - seg, 1e12),
        "full units first, shallow tiles first": np.where(ent > 0, -(ent >= 256).astype(float) * 1e9 + te, 1e12),
        "full units first, deep tiles first (descending)": np.where(ent > 0, -(ent >= 256).astype(float) * 1e9 - te, 1e12),
    }
    for name, k in keys.items():
        print(f"  replay, {name:68s}: {makespan(dur, np.argsort(k, kind='stable'), slots):5.1f} us")
    # what the walk time depends on
    for kd in sorted(set(kind.tolist())):
        m = (kind == kd) & (ent >= 256)
        if m.sum() < 20:
            continue
        print(f"  kind {kd}: full units {int(m.sum())}: walk vs tile list length  corr {np.corrcoef(te[m], walk[m])[0, 1]:+.2f};  by tile-length quartile: "
              + "  ".join(f"{np.mean(walk[m][(te[m] >= lo) & (te[m] <= hi)]):.1f}" for lo, hi in zip(np.quantile(te[m], [0, .25, .5, .75]), np.quantile(te[m], [.25, .5, .75, 1]))))
        if kd in (2, 4):
            print(f"          walk vs segment index corr {np.corrcoef(seg[m], walk[m])[0, 1]:+.2f}; vs (seg / nseg) {np.corrcoef(seg[m] / np.maximum(nseg[m], 1), walk[m])[0, 1]:+.2f}")
