"""Host time of the fused MLP nodes: the wall time of N forward + backward passes over ONE graph that holds every node of
tools/mlp_call_record.py (mlp2 stored and recomputing, the level node, both anchor-MLP nodes, anchor_gen) at its 37-row shapes,
where the device work is a few microseconds per launch and the host is all there is.  No device synchronisation inside the timed
region.

    python tools/mlp_host_time.py [N = 200]        one JSON line: seconds for N passes, weight gradients inline and deferred

To compare two trees, run this file of each tree in processes of their own, alternating (profiles/mlp_nodes_host_time.txt).
"""
import json
import sys
import time

import mlp_call_record as rec


def timed(mode, n):
    import torch
    from contextgs_amd import mlp
    torch.manual_seed(11)
    nodes = [rec.CASES[c]() for c in ("mlp2_stored", "mlp2_recompute", "level_both", "anchor_mlp3", "rows_keep1_tiled1_sub",
                                      "anchor_gen")]
    leaves = [t for _, ls in nodes for t in ls]

    def step():
        for t in leaves:
            t.grad = None
        sum(o.sum() for run, _ in nodes for o in run()).backward()

    prev = mlp.defer_weight_gradients(mode == "deferred")
    try:
        for _ in range(20):                 # the allocator has its blocks
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    finally:
        mlp.defer_weight_gradients(prev)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    print(json.dumps({"passes": n, **{f"{m}_s": round(timed(m, n), 6) for m in rec.MODES}}))
