"""Host time of the drop-in rasterizer's autograd node: the wall time of N forward + backward calls at the 64-Gaussian, 80x64
scene of tools/raster_call_record.py, where the device work is a few microseconds per launch and the host is all there is.

    python tools/raster_host_time.py [N = 200]        one JSON line: seconds for N calls of the plain and of the combined case

To compare two trees, run this file of each tree in processes of their own, alternating (profiles/raster_request.txt).
"""
import json
import sys
import time

from raster_call_record import build_call, run_call


def timed(case, n):
    import torch
    call = build_call(case, "visible")
    for _ in range(20):                 # the pair capacity settles, the allocator has its blocks
        run_call(*call, sync=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run_call(*call, sync=False)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    print(json.dumps({"calls": n, "plain_s": round(timed("plain", n), 6), "combined_s": round(timed("combined", n), 6)}))
