"""Timing of packed arrays on the GPU ("Value codecs").

A 256^3 float32 array stored as int16 under [scale_offset, cast_value, bytes,
crc32c] in 64^3 chunks, device-resident store:
  (a) one k_value_map launch in each direction over the read route's own items
      (one per chunk region of the 256^3 array): device events around the
      launch (so launch overhead is inside the figure, and the 100 MB working
      set fits the Infinity Cache), its bytes (2 + 4 per element) and TB/s;
  (b) Array.get(...) end to end (host clock around a call that ends in a
      device synchronise);
  (c) what a caller had before: the same store opened as a plain int16 array
      (bytes + crc32c), read with Array.get, then three torch kernels on the
      device (to float32, divide, add).
Medians after warm-up.  Prints one JSON line.

    python scripts/value_bench.py [--reps 20] [--profile]

--profile runs each map a few times and nothing else, for
`rocprofv3 --kernel-trace --stats -- python scripts/value_bench.py --profile`
(k_value_map's own time).
"""

import argparse
import json
import os
import statistics
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
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()

    import torch

    import zarr_hip
    from zarr_hip import _native as N
    from zarr_hip import values as V
    from zarr_hip.codecs import CastValueCodec, ScaleOffsetCodec
    from zarr_hip.pipeline import _stream_handle
    from zarr_hip.spec import ArraySpec

    if not torch.cuda.is_available():
        raise SystemExit("value_bench: no GPU (nothing is measured on the CPU)")
    dev = torch.device("cuda:0")
    n, c = args.n, args.chunk
    shape, chunks = (n, n, n), (c, c, c)
    so = {"name": "scale_offset", "configuration": {"offset": -2.5, "scale": 10}}
    cast = {"name": "cast_value", "configuration": {"data_type": "int16"}}
    tail = [{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "crc32c"}]
    rng = np.random.default_rng(0)
    stored = rng.integers(-30000, 30000, shape).astype(np.int16)

    store = zarr_hip.DeviceStore(dev, capacity=stored.nbytes * 2 + (64 << 20))
    plain = zarr_hip.Array.create(store, shape, chunks, "int16", 0, codecs=tail)
    plain[...] = stored
    packed = zarr_hip.Array.create(store, shape, chunks, "float32", 0.25, codecs=[so, cast] + tail)
    want = stored.astype(np.float32) / np.float32(10) + np.float32(-2.5)
    got = packed[...]
    if got.tobytes() != want.tobytes():
        raise SystemExit("value_bench: the packed read differs from numpy")

    # (a) the map alone, over one item per chunk region
    ops = V.ValueOps(ScaleOffsetCodec(offset=-2.5, scale=10), CastValueCodec("int16"),
                     ArraySpec(chunks, np.dtype("float32"), 0.25))
    S = torch.from_numpy(stored).to(dev)
    A = torch.empty(shape, dtype=torch.float32, device=dev)
    g = n // c

    def specs(asz, bsz):
        out = []
        for i in range(g):
            for j in range(g):
                for k in range(g):
                    e = (i * c * n + j * c) * n + k * c
                    out.append((e * asz, e * bsz, [(c, n * n * asz, n * n * bsz), (c, n * asz, n * bsz), (c, asz, bsz)],
                                0, 0))
        return out

    def prepared(op, sp, a, b, ne):
        items, prefix = V.make_items(sp)
        V._check_items(sp, V._extent(a), V._extent(b), a.element_size(), b.element_size())
        d_items = torch.from_numpy(items.view(np.uint8).reshape(-1)).to(dev)
        d_prefix = torch.from_numpy(prefix.view(np.int32)).to(dev)
        words = torch.zeros(1 + len(sp), dtype=torch.int32, device=dev)

        def go():
            V.launch(op, d_items, len(sp), d_prefix, int(prefix[-1]), None, a.data_ptr(), V._extent(a), b.data_ptr(),
                     V._extent(b), words, words[1:] if ne else None, _stream_handle(dev))
        return go, words

    dec, _ = prepared(ops.op(False), specs(2, 4), S, A, False)
    S2 = torch.empty_like(S)
    enc, words = prepared(ops.op(True), specs(4, 2), A, S2, True)
    dec()
    enc()
    torch.cuda.synchronize(dev)
    if A.cpu().numpy().tobytes() != want.tobytes() or int(words[0]) or not torch.equal(S, S2):
        raise SystemExit("value_bench: the map alone differs from numpy")
    if args.profile:
        for _ in range(5):
            dec()
            enc()
        torch.cuda.synchronize(dev)
        print(json.dumps({"profile": True, "last_kernel": N.lib().zhip_last_kernel().decode()}))
        return

    def events(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        return statistics.median(ts)

    def clock(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    nbytes = n ** 3 * 6
    t_dec, t_enc = events(dec), events(enc)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    t_get = clock(lambda: packed.get(Ellipsis, out=out))
    if out.cpu().numpy().tobytes() != want.tobytes():  # the timed reads (planned once, then replayed)
        raise SystemExit("value_bench: the timed packed read differs from numpy")
    out16 = torch.empty(shape, dtype=torch.int16, device=dev)

    def before():
        plain.get(Ellipsis, out=out16)
        return out16.to(torch.float32).div_(10.0).add_(-2.5)

    # (torch divides by a scalar as a multiplication by its reciprocal: close to numpy, not bit-equal)
    if not np.allclose(before().cpu().numpy(), want, rtol=1e-6, atol=1e-6):
        raise SystemExit("value_bench: the torch route differs from numpy")
    t_before = clock(before)
    t_plain = clock(lambda: plain.get(Ellipsis, out=out16))
    print(json.dumps({
        "array": f"{n}^3 float32 as int16, {c}^3 chunks, [scale_offset, cast_value, bytes, crc32c]",
        "reps": args.reps,
        "map_decode_s": t_dec, "map_decode_TBps": nbytes / t_dec / 1e12,
        "map_encode_s": t_enc, "map_encode_TBps": nbytes / t_enc / 1e12,
        "map_bytes": nbytes,
        "get_packed_s": t_get,
        "get_int16_then_torch_s": t_before,
        "get_int16_alone_s": t_plain,
    }))


if __name__ == "__main__":
    main()
