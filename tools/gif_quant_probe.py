"""GIF answers past 256 colours written on the device (IMPGPU_GIF_ENC_QUANTIZE) against the routes that exist without them,
in one session on the same albums:

    device   impgpu_batch_encode_gif_ex with the flag: eight launches a group, two waits, the finished files cross the link
    frames   (a) impgpu_batch_album_download of the same albums' 32-bit frames
    host     (b) = (a) + impgpu_gif_encode_host_ex (the same quantiser and encoder, the library's lane code) on ONE thread
    pillow   (c) = (a) + Pillow's quantize(256, MEDIANCUT, no dither) + tests/gif_writer.py: an OUTSIDE reference for what
             quantising costs a host.  gif_writer's LZW is Python, so (c) is split: "pillow_quantize_ms" is the part that
             says something.  Measured on ONE album and multiplied by the album count.

for a lone 640 x 480 one-frame album, an 8-frame 640 x 480 album and 64 albums of 8 frames at 320 x 240.  The frames are the
pixels of tests/golden/jpeg/c420_q50_640x480.jpg (halved by dropping pixels for 320 x 240) with a translucent overlay blended
in at a place of its own per frame: photo content with tens of thousands of colours.  Times are wall time of the call,
medians over --iters calls after a warm-up call, in ms; the routes are timed in two halves with the others in between.

"mse": the mean squared error of each case's first frame as the device wrote it (read back from the file) beside Pillow's
MEDIANCUT and FASTOCTREE at 256 colours without dither.

--kernel-stats: a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this probe (--only 8x640x480 --device-only)
made separately; the k_gif_enc_* rows are folded into the output as per-launch averages.

    timeout -k 10 900 python tools/gif_quant_probe.py [--iters 9] [--out profiles/gif_quant_probe.json]"""
import argparse
import csv
import ctypes as C
import io
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
LAUNCHES = 8


def photo():
    from PIL import Image

    return np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "jpeg", "c420_q50_640x480.jpg")).convert("RGB"))[..., ::-1]


def content(base, w, h, seed):
    """a BGRA frame: the photo (every second pixel of it at 320 x 240) under a translucent overlay"""
    rng = np.random.default_rng(seed)
    f = base[:: 480 // h, :: 640 // w][:h, :w].astype(np.int32)
    ow, oh = w // 3, h // 4
    x0, y0 = int(rng.integers(0, w - ow)), int(rng.integers(0, h - oh))
    yy, xx = np.mgrid[0:oh, 0:ow]
    overlay = np.stack([255 - xx * 255 // ow, yy * 255 // oh, np.full_like(xx, 40 + 20 * (seed % 8))], 2)
    f[y0: y0 + oh, x0: x0 + ow] = (f[y0: y0 + oh, x0: x0 + ow] * 5 + overlay * 3) // 8
    return np.ascontiguousarray(np.concatenate([f.astype(np.uint8), np.full((h, w, 1), 255, np.uint8)], 2))


def median_ms(fn, iters):
    fn()
    ts = []
    for _ in range(max(1, iters)):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def pillow_route(frames):
    """-> (file, seconds in quantize, seconds in gif_writer)"""
    from PIL import Image
    import gif_writer as G

    tq = tw = 0.0
    pages = []
    for f in frames:
        t0 = time.perf_counter()
        q = Image.fromarray(np.ascontiguousarray(f[..., 2::-1])).quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE)
        pal = np.frombuffer(bytes(q.getpalette()[: 768]).ljust(768, b"\0"), np.uint8).reshape(256, 3)
        idx = np.asarray(q)
        tq += time.perf_counter() - t0
        t0 = time.perf_counter()
        pages.append(G.make_page(idx, palette=pal, mcs=8))
        tw += time.perf_counter() - t0
    t0 = time.perf_counter()
    blob = G.write(pages, loop=True)
    tw += time.perf_counter() - t0
    return blob, tq, tw


def mse_row(blob, frame):
    from PIL import Image

    rgb = np.ascontiguousarray(frame[..., 2::-1])
    mse = lambda a: round(float(((np.asarray(a).astype(np.int64) - rgb.astype(np.int64)) ** 2).mean()), 2)
    im = Image.open(io.BytesIO(blob))
    im.seek(0)
    src = Image.fromarray(rgb)
    return {"device_file": mse(im.convert("RGB")),
            "pillow_mediancut": mse(src.quantize(256, method=Image.Quantize.MEDIANCUT, dither=Image.Dither.NONE).convert("RGB")),
            "pillow_fastoctree": mse(src.quantize(256, method=Image.Quantize.FASTOCTREE, dither=Image.Dither.NONE).convert("RGB"))}


def kernel_stats(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        if "k_gif_enc_" in r["Name"]:
            name = r["Name"][r["Name"].index("k_gif_enc_"):].split("(")[0]
            rows[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 1)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_quant_probe.json"))
    a = ap.parse_args()
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    base = photo()
    rows = []
    for name, w, h, frames, albums in CASES:
        if a.only and a.only != name:
            continue
        host_frames = [[content(base, w, h, 10 * k + f) for f in range(frames)] for k in range(min(albums, 4))]
        host_frames = [host_frames[k % len(host_frames)] for k in range(albums)]
        colours = len(np.unique(host_frames[0][0].reshape(-1, 4), axis=0))
        assert colours > 256
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
            rc = imp.lib.impgpu_batch_encode_gif_ex(handles, None, None, loops, n, a.segment, imp.GIF_ENC_QUANTIZE, outs, caps, lens, codes,
                                                    C.byref(launches))
            assert rc == 0 and not any(codes) and launches.value % LAUNCHES == 0, (rc, list(codes), launches.value)

        def download():
            rc = imp.lib.impgpu_batch_album_download(handles, n, datas, steps, codes)
            assert rc == 0 and not any(codes), (rc, list(codes))

        def host():
            download()
            for k in range(n):
                rc, blob, m, _ = imp.encode_gif_host(raw[k * frames: (k + 1) * frames], loop_count=0, segment=a.segment, capacity=bound, guard=0,
                                                     flags=imp.GIF_ENC_QUANTIZE)
                assert rc == 0 and m == lens[k], (rc, m, lens[k])

        device()
        for k in range(min(n, 4)):                                   # the files are the host encoder's, byte for byte
            rc, blob, m, _ = imp.encode_gif_host(host_frames[k], loop_count=0, segment=a.segment, flags=imp.GIF_ENC_QUANTIZE)
            assert rc == 0 and bufs[k][: lens[k]].tobytes() == blob
        h1, h2 = a.iters // 2, a.iters - a.iters // 2
        row = {"probe": "gif_quant", "case": name, "canvas": [w, h], "frames": frames, "albums": albums, "iters": a.iters,
               "segment": a.segment or imp.GIF_ENC_SEGMENT, "colours_of_first_frame": colours}
        if a.device_only:
            d1 = d2 = median_ms(device, a.iters)
        else:
            hi = max(1, min(a.iters, 3) // 2) if albums > 1 else h1  # (the host route takes seconds at 64 albums)
            d1, f1, c1 = median_ms(device, h1), median_ms(download, h1), median_ms(host, hi)
            c2, f2, d2 = median_ms(host, hi), median_ms(download, h2), median_ms(device, h2)
            download()
            blob, tq, tw = pillow_route(raw[:frames])
            file_bytes, frame_bytes = int(sum(lens)), n * frames * w * h * 4
            row.update({"frames_download_ms": round((f1 + f2) / 2, 3), "download_plus_host_encode_ms": round((c1 + c2) / 2, 3),
                        "frames_download_halves_ms": [round(f1, 3), round(f2, 3)], "download_plus_host_encode_halves_ms": [round(c1, 3), round(c2, 3)],
                        "pillow_quantize_ms": round(tq * 1e3 * albums, 1), "pillow_python_writer_ms": round(tw * 1e3 * albums, 1),
                        "pillow_route_is": "one album, one run, times the album count; the writer is Python",
                        "device_over_frames_download": round((d1 + d2) / (f1 + f2), 3), "host_route_over_device": round((c1 + c2) / (d1 + d2), 3),
                        "file_bytes": file_bytes, "pillow_file_bytes_one_album": len(blob), "frames_over_files": round(frame_bytes / file_bytes, 2),
                        "mse_first_frame": mse_row(bufs[0][: lens[0]].tobytes(), host_frames[0][0]),
                        "host_encoder": "impgpu_gif_encode_host_ex, one thread, the same quantiser (FreeImage is not installed)"})
        row.update({"launches": launches.value, "device_ms": round((d1 + d2) / 2, 3), "device_halves_ms": [round(d1, 3), round(d2, 3)]})
        rows.append(row)
        print(json.dumps(row), flush=True)
        for im in images:
            im.release()
    imp.env_destroy()
    result = {"rows": rows}
    if a.kernel_stats:
        result["per_launch_8x640x480"] = kernel_stats(a.kernel_stats)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
