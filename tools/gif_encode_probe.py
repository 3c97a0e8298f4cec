"""GIF answers written on the device against the route that exists without them, in one session on the same albums:

    device   impgpu_batch_encode_gif: five launches, two waits, the finished files cross the link
    frames   (a) impgpu_batch_album_download of the same albums' 32-bit frames: what a worker does today before it encodes
    host     (b) = (a) + impgpu_gif_encode_host for every album on ONE thread.  This stands in for FreeImage's SaveGIF, which
             is not installed: it is the library's own encoder (exact palette, no quantiser), so FreeImage's NNQUANT pass
             would come on top of it.

for a lone 640 x 480 one-frame album, an 8-frame 640 x 480 album and 64 albums of 8 frames at 320 x 240.  The frames are
"photo" content: smooth gradients plus noise over a 256-colour table, what a dithered picture looks like to LZW.  Times are
wall time of the call (every route's device work is complete when it returns), medians over --iters calls after a warm-up
call, in ms; every route is timed in two halves with the others in between, and both halves are written down.

"cut_cost": the file's size at segment 3584 / 8192 / 32768 over its size with no cut at all (one segment; checked here to be
gif_writer.lzw_encode's stream without clear_at), for 640 x 480 noise, photo and flat content.

--kernel-stats: a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this probe (--only 8x640x480) made
separately; the k_gif_enc_* rows are folded into the output as per-launch averages.

    timeout -k 10 900 python tools/gif_encode_probe.py [--iters 7] [--out profiles/gif_encode_probe.json]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [("1x640x480", 640, 480, 1, 1), ("8x640x480", 640, 480, 8, 1), ("64x8x320x240", 320, 240, 8, 64)]


def content(kind, w, h, seed):
    """a BGRA frame of at most 256 colours"""
    rng = np.random.default_rng(seed)
    pal = np.concatenate([rng.integers(0, 256, (256, 3), dtype=np.uint8), np.full((256, 1), 255, np.uint8)], 1)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        idx = rng.integers(0, 256, (h, w))
    elif kind == "photo":
        idx = ((xx + 2 * yy) // 6 + rng.integers(0, 12, (h, w))) & 255
    else:                                                            # flat: eight bands and a box
        idx = (yy * 8 // h) & 255
        idx[h // 4: h // 2, w // 4: w // 2] = 9
    return np.ascontiguousarray(pal[idx])


def median_ms(fn, iters):
    fn()
    ts = []
    for _ in range(max(1, iters)):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def cut_cost(imp):
    from test_gif_encode_host import model_file, model_pages

    out = {}
    for kind in ("noise", "photo", "flat"):
        f = content(kind, 640, 480, 3)
        rc, whole, n, _ = imp.encode_gif_host([f], segment=1 << 24)
        assert rc == 0
        if kind == "photo":                                          # "no cut" is gif_writer's stream without clear_at
            assert model_pages([f], segment=1 << 24)[0][0]["clear_at"] == () and whole == model_file([f], segment=1 << 24)
        row = {"no_cut_bytes": n}
        for seg in (3584, 8192, 32768):
            rc, blob, m, _ = imp.encode_gif_host([f], segment=seg)
            assert rc == 0
            row["segment_%d" % seg] = {"bytes": m, "over_no_cut": round(m / n, 4)}
        out[kind] = row
    return out


def kernel_stats(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        if "k_gif_enc_" in r["Name"]:
            name = r["Name"][r["Name"].index("k_gif_enc_"):].split("(")[0]
            rows[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 1)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_encode_probe.json"))
    a = ap.parse_args()
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    rows = []
    for name, w, h, frames, albums in CASES:
        if a.only and a.only != name:
            continue
        host_frames = [[content("photo", w, h, 10 * k + f) for f in range(frames)] for k in range(min(albums, 4))]
        host_frames = [host_frames[k % len(host_frames)] for k in range(albums)]
        images = [imp.Image.album(fr) for fr in host_frames]
        n = albums
        handles = (C.c_void_p * n)(*[im.h.value for im in images])
        bound = imp.gif_encode_bound(w, h, frames)
        bufs = [np.empty(bound, np.uint8) for _ in range(n)]
        outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        caps, lens, codes, launches = (C.c_size_t * n)(*[bound] * n), (C.c_size_t * n)(), (C.c_int * n)(), C.c_int()
        loops = (C.c_int * n)(*[0] * n)
        raw = [np.empty((h, w, 4), np.uint8) for _ in range(n * frames)]
        datas = (C.c_void_p * (n * frames))(*[r.ctypes.data for r in raw])
        steps = (C.c_int * (n * frames))(*[w * 4] * (n * frames))

        def device():
            rc = imp.lib.impgpu_batch_encode_gif(handles, None, None, loops, n, a.segment, outs, caps, lens, codes, C.byref(launches))
            assert rc == 0 and not any(codes) and launches.value == 5, (rc, list(codes), launches.value)

        def download():
            rc = imp.lib.impgpu_batch_album_download(handles, n, datas, steps, codes)
            assert rc == 0 and not any(codes), (rc, list(codes))

        def host():
            download()
            for k in range(n):
                rc, blob, m, _ = imp.encode_gif_host(raw[k * frames: (k + 1) * frames], loop_count=0, segment=a.segment, capacity=bound, guard=0)
                assert rc == 0 and m == lens[k], (rc, m, lens[k])

        device()
        for k in range(min(n, 4)):                                   # the files are the host encoder's, byte for byte
            rc, blob, m, _ = imp.encode_gif_host(host_frames[k], loop_count=0, segment=a.segment)
            assert rc == 0 and bufs[k][: lens[k]].tobytes() == blob
        h1, h2 = a.iters // 2, a.iters - a.iters // 2
        hi = max(1, min(a.iters, 3) // 2) if albums > 1 else h1      # (the host route takes seconds at 64 albums)
        d1, f1, c1 = median_ms(device, h1), median_ms(download, h1), median_ms(host, hi)
        c2, f2, d2 = median_ms(host, hi), median_ms(download, h2), median_ms(device, h2)
        file_bytes, frame_bytes = int(sum(lens)), n * frames * w * h * 4
        row = {"probe": "gif_encode", "case": name, "canvas": [w, h], "frames": frames, "albums": albums, "iters": a.iters,
               "segment": a.segment or imp.GIF_ENC_SEGMENT, "launches": launches.value,
               "device_ms": round((d1 + d2) / 2, 3), "frames_download_ms": round((f1 + f2) / 2, 3), "download_plus_host_encode_ms": round((c1 + c2) / 2, 3),
               "device_halves_ms": [round(d1, 3), round(d2, 3)], "frames_download_halves_ms": [round(f1, 3), round(f2, 3)],
               "download_plus_host_encode_halves_ms": [round(c1, 3), round(c2, 3)],
               "device_over_frames_download": round((d1 + d2) / (f1 + f2), 3), "host_route_over_device": round((c1 + c2) / (d1 + d2), 3),
               "link_bytes_device_route": file_bytes + 32 * n * frames + 1024 * n, "link_bytes_frames_route": frame_bytes,
               "file_bytes": file_bytes, "frames_over_files": round(frame_bytes / file_bytes, 2),
               "host_encoder": "impgpu_gif_encode_host, one thread, exact palette (FreeImage is not installed)"}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for im in images:
            im.release()
    imp.env_destroy()
    result = {"rows": rows}
    if not a.only:
        result["cut_cost_640x480"] = cut_cost(imp)
        print(json.dumps(result["cut_cost_640x480"]), flush=True)
    if a.kernel_stats:
        result["per_launch_8x640x480"] = kernel_stats(a.kernel_stats)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
