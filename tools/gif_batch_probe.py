"""GIF compose in batches on one device -> one JSON line per row: ONE impgpu_batch_gif_compose call over `count` files against
the loop of impgpu_gif_compose_album calls over the same files (the only path before the batch call existed and unchanged by
it, so it is the baseline, taken in the same process).  Times are wall time from the call to the end of the device's work
(impgpu_sync inside the timed region: both forms only enqueue), medians over --iters calls after warm-up, microseconds,
the two forms interleaved in halves so that a drift of the machine lands on both.
  pools: small -- 64 GIFs of 200 x 200, 10 pages;  large -- 16 GIFs of 500 x 400, 30 pages
  (page 0 is the canvas, later pages are sub-rectangles as an encoder's frame differencing leaves them)

    timeout -k 10 600 python tools/gif_batch_probe.py [--iters 30] [--out rows.jsonl]
`--broker` times the same files as IMPB_IN_GIF requests (resize=100,0, every frame back) through an impgpu_broker at 1 and 8
client threads instead, requests per second over --seconds:
    timeout -k 10 600 python tools/gif_batch_probe.py --broker [--seconds 3] [--out rows.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POOLS = {"small": (64, 200, 200, 10), "large": (16, 500, 400, 30)}


def gif_pages(seed, cw, ch, n):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (256, 4), dtype=np.uint8)
    pages = []
    for f in range(n):
        w, h = (cw, ch) if f == 0 else (int(rng.integers(cw // 4, cw + 1)), int(rng.integers(ch // 4, ch + 1)))
        left, top = (0, 0) if f == 0 else (int(rng.integers(0, cw - w + 1)), int(rng.integers(0, ch - h + 1)))
        idx = np.zeros((h, (w + 3) & ~3), np.uint8)
        idx[:, :w] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        pages.append({"indices": idx, "width": w, "left": left, "top": top, "dispose": int(rng.integers(0, 4)), "key": 255, "palette": pal})
    return pages


def pool(name):
    count, cw, ch, n = POOLS[name]
    return [gif_pages(7000 + k, cw, ch, n) for k in range(count)]


def median_us(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e6


def library_rows(iters):
    import ngx_http_imgproc_amd as imp
    from ngx_http_imgproc_amd._lib import CGifSet

    imp.env_start(0)
    rows = []
    for name in POOLS:
        files = pool(name)
        n = len(files)
        arrays = [imp.gif_page_array(p) for p in files]              # the C calls on prebuilt arrays: the library, not the wrapper
        sets = (CGifSet * n)()
        for i, (arr, _) in enumerate(arrays):
            sets[i].pages, sets[i].count, sets[i].destructive, sets[i].page = arr, len(files[i]), 1, -1
        outs, codes, launches, one = (C.c_void_p * n)(), (C.c_int * n)(), C.c_int(), C.c_void_p()

        def batch():
            rc = imp.lib.impgpu_batch_gif_compose(sets, n, outs, codes, C.byref(launches))
            assert rc == 0 and not any(codes), (rc, list(codes))
            imp.sync()
            for i in range(n):
                imp.lib.impgpu_image_release(C.byref(C.c_void_p(outs[i])))

        def loop():
            got = []
            for i, (arr, _) in enumerate(arrays):
                rc = imp.lib.impgpu_gif_compose_album(arr, len(files[i]), 1, -1, C.byref(one))
                assert rc == 0, rc
                got.append(one.value)
            imp.sync()
            for h in got:
                imp.lib.impgpu_image_release(C.byref(C.c_void_p(h)))

        b1, l1 = median_us(batch, iters // 2), median_us(loop, iters // 2)
        l2, b2 = median_us(loop, iters - iters // 2), median_us(batch, iters - iters // 2)
        count, cw, ch, pages = POOLS[name]
        rows.append({"probe": "gif_batch", "pool": name, "files": count, "canvas": [cw, ch], "pages": pages, "iters": iters,
                     "batch_us": round((b1 + b2) / 2, 1), "loop_us": round((l1 + l2) / 2, 1), "batch_halves_us": [round(b1, 1), round(b2, 1)],
                     "loop_halves_us": [round(l1, 1), round(l2, 1)], "speedup": round((l1 + l2) / (b1 + b2), 3), "launches": launches.value})
    imp.env_destroy()
    return rows


def broker_rows(seconds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import worker_scaling
    from ngx_http_imgproc_amd import broker as B

    name = "/impgpu-gif-probe-%d" % os.getpid()
    p = worker_scaling.start_broker(name, threads=2, gather_us=0, slots=16, extra=["--slot-mb", "40"])
    rows = []
    try:
        for pool_name in POOLS:
            files = pool(pool_name)
            for clients in (1, 8):
                cs = [B.Client(name) for _ in range(clients)]
                done, sizes = [0] * clients, [[] for _ in range(clients)]
                for c in cs:                                            # warm: every size once
                    assert c.run(gif_pages=files[0], destructive=1, resize="100,0", simple=1, out=B.OUT_FRAME)[:2] == (0, 0)
                t_end = time.perf_counter() + seconds

                def work(k):
                    i = k
                    while time.perf_counter() < t_end:
                        rc, code, step, got, a = cs[k].run(gif_pages=files[i % len(files)], destructive=1, resize="100,0", simple=1, out=B.OUT_FRAME)
                        assert (rc, code) == (0, 0), (rc, code, step)
                        sizes[k].append(a.batch_size)
                        done[k] += 1
                        i += clients
                t0 = time.perf_counter()
                ts = [threading.Thread(target=work, args=(k,)) for k in range(clients)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                dt = time.perf_counter() - t0
                every = [b for s in sizes for b in s]
                rows.append({"probe": "gif_broker", "pool": pool_name, "clients": clients, "seconds": round(dt, 2), "requests": sum(done),
                             "requests_per_s": round(sum(done) / dt, 1), "mean_batch": round(sum(every) / max(1, len(every)), 2)})
                for c in cs:
                    c.close()
    finally:
        err = worker_scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--broker", action="store_true")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = broker_rows(a.seconds) if a.broker else library_rows(a.iters)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
