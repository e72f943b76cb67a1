"""Timing of orthogonal and coordinate selections on the GPU (DESIGN.md,
"Non-basic selections").

A 256^3 float32 array in 64^3 chunks (bytes + crc32c), device-resident store:
  (i)  oindex with a full-length permuted index on dimension 0 (dense: 2^24
       elements, affine inner dimensions);
  (ii) vindex of 10^6 random points;
  (iii) the same points as device tensors, planned on the device
       (zarr_hip.points): Array.get end to end, the device-event time of
       count + fill + gather, and the host clock of the planning at a tenth of
       the points and at all of them;
  (iv) case (i) with the permutation as a device tensor, planned per axis on
       the device (zarr_hip.axes);
  (v)  10^6 random row ids with repeats on dimension 0 and 0:4 on the other
       two, once with host ids and once with device ids.
       For (iv) and (v): Array.get end to end on both routes of the same run,
       the device-event time of count + fill + gather, and the host clock of
       planning + gather at a tenth of the ids and at all of them.
For (i) and (ii): Array.get(...) end to end (host clock around a call that ends in a
device synchronise), and the gather launch alone (device events around
SelectTables.launch: the table upload and k_select_copy) with its bytes per
second.  Next to them, on the same build: the basic full read arr.get(...),
and what a caller had to do before -- a full read to the host followed by
numpy fancy indexing.

    python scripts/fancy_bench.py [--reps 20] [--profile]

--profile runs each gather a few times and nothing else, for
`rocprofv3 --kernel-trace --stats -- python scripts/fancy_bench.py --profile`
(k_select_copy's, k_points_count's and k_points_fill's own times).  Prints one
JSON line.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zarr-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()

    import torch

    import zarr_hip
    from zarr_hip import buffer, fancy
    from zarr_hip.indexing import CoordinateIndexer, OrthogonalIndexer

    if not torch.cuda.is_available():
        raise SystemExit("fancy_bench: no GPU (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    n, c = args.n, args.chunk
    shape, chunks = (n, n, n), (c, c, c)
    rng = np.random.default_rng(0)
    data = rng.standard_normal(shape, dtype=np.float32)
    store = zarr_hip.DeviceStore(dev, capacity=data.nbytes + (64 << 20))
    arr = zarr_hip.Array.create(store, shape, chunks, "float32", 0.0,
                                codecs=[{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "crc32c"}])
    arr[...] = data
    perm = rng.permutation(n)
    pts = tuple(rng.integers(0, n, args.points) for _ in range(3))
    sels = {"oindex_perm_dim0": (perm, slice(None), slice(None)), "vindex_points": pts}
    want = {"oindex_perm_dim0": data[perm], "vindex_points": data[pts]}

    def sync():
        torch.cuda.synchronize(dev)

    def wall(fn, reps):
        fn()
        sync()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t)
        return float(np.median(ts) * 1e3), float(np.min(ts) * 1e3)

    def gather_tables(sel, out, scratch):
        """The tables the read route builds for this selection (all items in one launch)."""
        ix = (OrthogonalIndexer if isinstance(sel[1], slice) else CoordinateIndexer)(sel, shape, chunks)
        isz = 4
        cstr = [c * c * isz, c * isz, isz]
        tabs = fancy.SelectTables(isz, fancy.tensor_extent(scratch), fancy.tensor_extent(out))
        elems = 0
        grid = (n // c,) * 3
        for co, csel, osel, _ in ix:
            j = int(np.ravel_multi_index(co, grid))  # the chunk's slot in `scratch`
            nz = fancy.normalize(csel, osel, ix.drop_axes, chunks, tuple(out.shape))
            tabs.add(nz, j * c * c * c * isz, cstr, 0, [int(s) * isz for s in out.stride()])
            elems += nz.total
        return tabs, elems

    res = {"shape": shape, "chunks": chunks, "dtype": "float32", "reps": args.reps}
    full = arr.get((Ellipsis,))  # the decoded array: the scratch the gather reads
    scratch = torch.cat([full[i:i + c, j:j + c, k:k + c].reshape(c, c, c) for i in range(0, n, c)
                         for j in range(0, n, c) for k in range(0, n, c)], 0).contiguous()
    for name, sel in sels.items():
        got = buffer.to_numpy(arr.get(sel), np.float32)
        if got.tobytes() != np.ascontiguousarray(want[name]).tobytes():
            raise SystemExit(f"fancy_bench: {name} differs from numpy")
        out = torch.empty(want[name].shape, dtype=torch.float32, device=dev)
        tabs, elems = gather_tables(sel, out, scratch)
        if args.profile:
            for _ in range(5):
                keep = tabs.launch(scratch, out, dev)
            sync()
            continue
        keep = tabs.launch(scratch, out, dev)
        sync()
        if buffer.to_numpy(out, np.float32).tobytes() != np.ascontiguousarray(want[name]).tobytes():
            raise SystemExit(f"fancy_bench: {name}: the timed gather differs from numpy")
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            keep = tabs.launch(scratch, out, dev)
            b.record()
        sync()
        ms = float(np.median([a.elapsed_time(b) for a, b in ev]))
        table_bytes = tabs.pairs * 16
        moved = elems * 8 + table_bytes  # each element read and written once, each table pair read once
        e2e = wall(lambda: arr.get(sel), args.reps)
        res[name] = {"elements": elems, "gather_launch_ms": ms, "bytes_moved": moved,
                     "gather_GBps": moved / ms / 1e6, "table_bytes": table_bytes,
                     "get_ms_median": e2e[0], "get_ms_min": e2e[1]}
        del keep
    # (iii) the points of (ii) as device tensors: planned on the device (zarr_hip.points)
    from zarr_hip.points import DeviceCoordinateIndexer

    isz = 4
    cstr = [c * c * isz, c * isz, isz]
    slot_bytes = c * c * c * isz

    def device_plan_and_gather(dsel, out):
        """count (+ the one readback) + fill + gather against the decoded scratch."""
        ix = DeviceCoordinateIndexer(dsel, shape, chunks)
        table = ix.build_table(cstr, isz, False)
        tabs = fancy.SelectTables(isz, fancy.tensor_extent(scratch), fancy.tensor_extent(out))
        for k, rix in enumerate(ix.chunk_rixs):
            tabs.add_points(int(ix.counts[k]), int(ix.first[k]), int(rix) * slot_bytes, slot_bytes, (ix.n - 1) * isz)
        return tabs.launch(scratch, out, dev, table=table), table

    dpts = tuple(torch.from_numpy(p).to(dev) for p in pts)
    got = arr.get(dpts)
    if not got.is_cuda or buffer.to_numpy(got, np.float32).tobytes() != np.ascontiguousarray(want["vindex_points"]).tobytes():
        raise SystemExit("fancy_bench: vindex_points_device differs from numpy")
    out = torch.empty(args.points, dtype=torch.float32, device=dev)
    keep = device_plan_and_gather(dpts, out)
    sync()
    if buffer.to_numpy(out, np.float32).tobytes() != np.ascontiguousarray(want["vindex_points"]).tobytes():
        raise SystemExit("fancy_bench: vindex_points_device: the timed plan + gather differs from numpy")
    if args.profile:
        for _ in range(5):
            keep = device_plan_and_gather(dpts, out)
        sync()
    else:
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            keep = device_plan_and_gather(dpts, out)
            b.record()
        sync()
        e2e = wall(lambda: arr.get(dpts), args.reps)
        r3 = {"elements": args.points, "get_ms_median": e2e[0], "get_ms_min": e2e[1],
              "count_fill_gather_event_ms": float(np.median([a.elapsed_time(b) for a, b in ev]))}
        # the host section against the point count: planning (count launch, the readback, the items) on the host
        # clock, for a tenth of the points and for all of them -- per-point host work would show as a tenfold step
        for frac in (10, 1):
            sub = tuple(t[: args.points // frac].contiguous() for t in dpts)
            sub_out = out[: args.points // frac]
            p = wall(lambda: device_plan_and_gather(sub, sub_out), args.reps)
            r3[f"plan_and_gather_wall_ms_{args.points // frac}_points"] = {"median": p[0], "min": p[1]}
        res["vindex_points_device"] = r3
    del keep
    # (iv), (v): orthogonal selections whose index array is a device tensor, planned per axis on the device
    # (zarr_hip.axes), next to the host-index route of the same run
    from zarr_hip.axes import DeviceOrthogonalIndexer

    grid = (n // c,) * 3

    def axes_plan_and_gather(dsel, out):
        """count (+ the one readback) + fill + gather against the decoded scratch."""
        ix = DeviceOrthogonalIndexer(dsel, shape, chunks)
        ostr = [int(s) * isz for s in out.stride()]
        table = ix.build_table(cstr, ostr, False)
        tabs = fancy.SelectTables(isz, fancy.tensor_extent(scratch), fancy.tensor_extent(out))
        for it in ix.items():
            tabs.add_product(it.dims, int(np.ravel_multi_index(it.coords, grid)) * slot_bytes, cstr, ostr)
        return tabs.launch(scratch, out, dev, table=table), table

    ids = rng.integers(0, n, args.rows)  # with repeats
    ortho = {"oindex_perm_dim0_device": (perm, slice(None), slice(None)),
             "oindex_rows_repeats": (ids, slice(0, 4), slice(0, 4))}
    for name, sel in ortho.items():
        dsel = (torch.from_numpy(sel[0]).to(dev),) + sel[1:]
        expect = np.ascontiguousarray(data[sel[0]][:, sel[1], sel[2]])
        got = arr.get(dsel)
        if not got.is_cuda or buffer.to_numpy(got, np.float32).tobytes() != expect.tobytes():
            raise SystemExit(f"fancy_bench: {name} differs from numpy")
        out = torch.empty(expect.shape, dtype=torch.float32, device=dev)
        keep = axes_plan_and_gather(dsel, out)
        sync()
        if buffer.to_numpy(out, np.float32).tobytes() != expect.tobytes():
            raise SystemExit(f"fancy_bench: {name}: the timed plan + gather differs from numpy")
        if args.profile:
            for _ in range(5):
                keep = axes_plan_and_gather(dsel, out)
            sync()
            continue
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            keep = axes_plan_and_gather(dsel, out)
            b.record()
        sync()
        dev_get = wall(lambda: arr.get(dsel), args.reps)
        host_get = wall(lambda: arr.get(sel), args.reps)
        r = {"elements": int(expect.size), "ids": int(len(sel[0])),
             "device_ids_get_ms": {"median": dev_get[0], "min": dev_get[1]},
             "host_ids_get_ms": {"median": host_get[0], "min": host_get[1]},
             "count_fill_gather_event_ms": float(np.median([a.elapsed_time(b) for a, b in ev]))}
        # planning + gather on the host clock at a tenth of the ids and at all of them: per-index host work
        # would show as a tenfold step
        for frac in (10, 1):
            k = len(sel[0]) // frac
            sub = (dsel[0][:k].contiguous(),) + sel[1:]
            sub_out = out[:k]
            p = wall(lambda: axes_plan_and_gather(sub, sub_out), args.reps)
            r[f"plan_and_gather_wall_ms_{k}_ids"] = {"median": p[0], "min": p[1]}
        res[name] = r
        del keep
    if not args.profile:
        b = wall(lambda: arr.get((Ellipsis,)), args.reps)
        res["basic_full_get_ms"] = {"median": b[0], "min": b[1]}
        h = wall(lambda: arr[...], max(3, args.reps // 4))
        res["full_read_to_host_ms"] = {"median": h[0], "min": h[1]}
        host = arr[...]
        for name, sel in sels.items():
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                host[sel]
                ts.append(time.perf_counter() - t)
            res[name]["numpy_fancy_on_host_ms"] = float(np.median(ts) * 1e3)
            res[name]["host_route_total_ms"] = res["full_read_to_host_ms"]["median"] + res[name]["numpy_fancy_on_host_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
