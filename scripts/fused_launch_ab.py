#!/usr/bin/env python
"""Same-process A/B of the fused launch on the headline batch (measurement only).

The headline replicas (bench.py's: 256^3 float32 in 128^3 shards of 64^3 inner
chunks, 4 independent replicas) are captured twice as a ReadGraph of STEPS
decodes -- fuse=False (one k_decode_il launch per decode) and fuse=True (up to
zhip_multi_max() decodes per launch, k_decode_il_multi) -- and replayed in
interleaved pairs, event-timed on the launch stream as bench.py's graph_steps
times its loop.  One JSON line per arm with every reading (microseconds per
decode), then one summary line: the medians, the gain, and each arm's spread
(max - min over its repeats), which the gain has to be set against.  The
shipped library; results are checked after every replay.

Environment: STEPS (20), PAIRS (7), WARM (3 replays per arm before timing)."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zarr-python_amd"))

import bench  # noqa: E402
import workloads as W  # noqa: E402


def main():
    import torch

    import zarr_hip
    from zarr_hip import _native as N

    dev = torch.device("cuda:0")
    steps = int(os.environ.get("STEPS", "20"))
    pairs = int(os.environ.get("PAIRS", "7"))
    warm = int(os.environ.get("WARM", "3"))
    g = W.HEADLINE
    data = torch.from_numpy(W.synthetic(g["shape"])).to(dev)
    reps = [bench.build_replica(dev, data, g["shape"], g["inner"], [W.LE, W.CRC], shards=g["shards"])
            .prepare_read((Ellipsis,)) for _ in range(4)]
    progs = [p for p, _ in reps]
    graphs = {"unfused": zarr_hip.ReadGraph(progs, steps, dev, fuse=False),
              "fused": zarr_hip.ReadGraph(progs, steps, dev, fuse=True)}
    kernel = N.lib().zhip_last_kernel().decode()
    stream = torch.cuda.current_stream(dev)

    def once(gr) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        a.record(stream)
        gr.replay()
        b.record(stream)
        torch.cuda.synchronize(dev)
        for p in progs:
            p.results()
        return a.elapsed_time(b) * 1e3 / steps  # us per decode

    want = data.view(torch.int32)
    for name, gr in graphs.items():
        for _, out in reps:
            out.zero_()
        for _ in range(warm):
            once(gr)
        for _, out in reps[: min(4, steps)]:
            assert torch.equal(out.view(torch.int32), want), f"{name}: decoded bytes differ from the source"
    us = {name: [] for name in graphs}
    for i in range(pairs):
        for name in (("unfused", "fused") if i % 2 == 0 else ("fused", "unfused")):
            us[name].append(once(graphs[name]))
    med = {k: float(np.median(v)) for k, v in us.items()}
    spread = {k: float(max(v) - min(v)) for k, v in us.items()}
    for name, gr in graphs.items():
        print(json.dumps({"arm": name, "kernel": kernel, "steps": steps, "launches": gr.launches,
                          "us_per_decode": [round(x, 3) for x in us[name]], "median": round(med[name], 3),
                          "min": round(min(us[name]), 3), "spread": round(spread[name], 3)}), flush=True)
    gain = med["unfused"] - med["fused"]
    print(json.dumps({"summary": "fused vs unfused", "device": torch.cuda.get_device_name(dev),
                      "gain_us": round(gain, 3), "gain_pct": round(100 * gain / med["unfused"], 2),
                      "worst_spread_us": round(max(spread.values()), 3),
                      "gain_over_spread": round(gain / max(max(spread.values()), 1e-9), 2),
                      "every_fused_below_every_unfused": max(us["fused"]) < min(us["unfused"])}), flush=True)


if __name__ == "__main__":
    main()
