"""Host time of zhip_plan_create + zhip_plan_upload for the headline layout
(inner chunk 64^3 float32 of a sharded 256^3 array, CRC): median of repeated
calls in one process.  Usage: plan_host_time.py ROOT  (ROOT: tree whose library to load)."""
import ctypes
import json
import os
import statistics
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path[:0] = [root, os.path.join(root, "zarr-python_amd")]
import torch  # noqa: E402
from zarr_hip import _native as N  # noqa: E402

assert N.__file__.startswith(root), N.__file__
torch.cuda.init()
L = N.Layout()
L.ndim, L.itemsize = 3, 4
for d, (s, o) in enumerate(zip((64, 64, 64), (256 * 256 * 4, 256 * 4, 4))):
    L.shape[d], L.out_stride[d] = s, o
L.nbytes = 64 * 64 * 64 * 4
L.flags = N.LF_CRC | N.LF_SHARDED | N.LF_FLOAT
L.n_inner, L.index_size = 8, 16 * 8 + 4
lib = N.lib()
create, upload, total = [], [], []
for it in range(25):
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    N.check(lib.zhip_plan_create(ctypes.byref(L), ctypes.byref(h)), "create")
    t1 = time.perf_counter()
    N.check(lib.zhip_plan_upload(h), "upload")
    t2 = time.perf_counter()
    lib.zhip_plan_destroy(h)
    if it >= 5:  # warm-up: first allocations
        create.append((t1 - t0) * 1e3)
        upload.append((t2 - t1) * 1e3)
        total.append((t2 - t0) * 1e3)
med = statistics.median
print(json.dumps({"tree": sys.argv[1], "n": len(total), "create_ms_median": round(med(create), 3),
                  "upload_ms_median": round(med(upload), 3), "total_ms_median": round(med(total), 3),
                  "total_ms_min": round(min(total), 3), "total_ms_max": round(max(total), 3)}))
