"""Measurements of the device's decode of lossy WebP uploads with alpha (impgpu_batch_decode_webp_ex with
IMPGPU_WEBP_ACCEPT_LOSSY | IMPGPU_WEBP_ACCEPT_ALPHA) -> profiles/webp_alpha_decode_probe.json.

    python tools/webp_alpha_decode_probe.py [--out FILE]
                                                     needs the device: per case, interleaved in one session, medians after a
                                                     warm-up of (1) the call with accept=3, (2) the same files' bare `VP8 `
                                                     chunks with accept=1 -- the difference is what alpha costs -- and
                                                     (3) Pillow's decode on one core plus impgpu_image_upload
    python tools/webp_alpha_decode_probe.py --trace  every trace case twice, to be run under
                                                     `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/webp_alpha_decode_probe.py --trace`
    python tools/webp_alpha_decode_probe.py --fold CSV [--out FILE]
                                                     CPU only: the per-kernel times of such a run's kernel_trace.csv into the file

Cases: a lone 640x480 file, a lone 1920x1080 file, 64 files of 320x240 (tools/webp_encode_probe.py's photo-like frames as
the colour plane), each with (a) a soft-edged mask as alpha and (b) a noise alpha, written by Pillow at quality 75, and
(c) the mask of (a) hand-assembled as a gradient-filtered VP8L plane around the same `VP8 ` chunk
(tests/webp_alpha_dec_cases.py).  The trace adds the mask under each of the four filters, so that k_webp_alpha's time per
filter stands next to k_vp8_dec_recon's.
"""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import webp_alpha_dec_cases as C  # noqa: E402
from webp_encode_probe import GEOMETRIES, frames_of  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "webp_alpha_decode_probe.json")
KERNELS = ("k_vp8_dec_recon", "k_vp8_dec_filter", "k_vp8_dec_frame", "k_webp_dec_tables", "k_webp_dec_pixels", "k_webp_dec_inverse", "k_webp_alpha")
VARIANTS = ("mask", "noise", "mask_gradient")
TRACE_VARIANTS = ("mask", "noise", "mask_none", "mask_horizontal", "mask_vertical", "mask_gradient")


def pillow_file(bgra):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])).save(buf, format="WEBP", quality=75)
    return buf.getvalue()


def pillow_bgra(blob):
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    im.load()
    return np.ascontiguousarray(np.asarray(im.convert("RGBA"))[..., [2, 1, 0, 3]])


def files_of(geometry, variant):
    """-> (the files, their bare `VP8 ` chunks as files)"""
    w, h, _ = GEOMETRIES[geometry]
    files = []
    for k, f in enumerate(frames_of(geometry, "photo")):
        f = f.copy()
        f[..., 3] = C.plane("noise" if variant == "noise" else "mask", w, h, k)
        blob = pillow_file(f)
        if variant.startswith("mask_"):                      # the plane Pillow's own file decodes to, under the filter asked for
            a = pillow_bgra(blob)[..., 3]
            blob = C.alpha_file(C.vp8_payload(blob), w, h, C.alph(a, C.FILTERS.index(variant[5:]), method=1))
        files.append(blob)
    return files, [C.riff(C.chunk(b"VP8 ", C.vp8_payload(b))) for b in files]


def measure(out_path):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    rows = []
    for g in GEOMETRIES:
        for variant in VARIANTS:
            blobs, bare = files_of(g, variant)
            reps = 3 if GEOMETRIES[g][0] >= 1920 else 5

            def device(files, accept):
                res, launches = imp.batch_decode_webp(files, accept=accept)
                for rc, im in res:
                    assert rc == 0, rc
                    im.release()
                return launches

            def host():
                for b in blobs:
                    imp.Image(pillow_bgra(b)).release()
                imp.sync()

            res, launches = imp.batch_decode_webp(blobs, accept=3)
            same = all(rc == 0 and np.array_equal(im.numpy(), pillow_bgra(b)) for (rc, im), b in zip(res, blobs))
            for _, im in res:
                im.release()
            runs = {"alpha": lambda: device(blobs, 3), "bare": lambda: device(bare, 1), "host": host}
            times = {k: [] for k in runs}
            for fn in runs.values():                         # the warm-up
                fn()
            for _ in range(reps):                            # interleaved
                for k, fn in runs.items():
                    t = time.perf_counter()
                    fn()
                    times[k].append((time.perf_counter() - t) * 1e3)
            info = imp.webp_alpha_info(blobs[0])[1]
            row = {"geometry": g, "variant": variant, "files": len(blobs), "file_bytes": sum(len(b) for b in blobs), "alph_bytes": sum(len(C.find_chunk(b, b"ALPH")) for b in blobs),
                   "alph_header": "%02x" % C.find_chunk(blobs[0], b"ALPH")[0], "alpha_feature_word": info[3], "launches": launches, "frames_equal_pillow": bool(same),
                   "accept3_ms": float(np.median(times["alpha"])), "bare_vp8_accept1_ms": float(np.median(times["bare"])),
                   "pillow_plus_upload_ms": float(np.median(times["host"]))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    imp.env_destroy()
    doc = {"what": "impgpu_batch_decode_webp_ex with accept=3 on VP8X + ALPH + VP8 files against the same files' bare VP8 chunks with accept=1 and against "
                   "Pillow's decode on one core + impgpu_image_upload; interleaved, medians, one session", "rows": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def trace():
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    for g in GEOMETRIES:
        for variant in TRACE_VARIANTS:
            blobs, _ = files_of(g, variant)
            for _ in range(2):                               # a warm-up, then the call the fold reads (the LAST of each case)
                res, _ = imp.batch_decode_webp(blobs, accept=3)
                for rc, im in res:
                    assert rc == 0, rc
                    im.release()
    imp.env_destroy()


def fold(csv_path, out_path):
    """every call ends with its one k_webp_alpha launch; two calls a case: the second call's durations, in microseconds"""
    import csv

    with open(csv_path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name = [k for k in KERNELS if k in r["Kernel_Name"]][0]
        cur[name] = cur.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if name == "k_webp_alpha":
            calls.append(cur)
            cur = {}
    cases = [(g, v) for g in GEOMETRIES for v in TRACE_VARIANTS]
    assert len(calls) == 2 * len(cases), len(calls)
    with open(out_path) as f:
        doc = json.load(f)
    doc["kernel_us"] = [{"geometry": g, "variant": v, **calls[2 * k + 1]} for k, (g, v) in enumerate(cases)]
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    if "--trace" in sys.argv:
        trace()
    elif "--fold" in sys.argv:
        fold(sys.argv[sys.argv.index("--fold") + 1], out)
    else:
        measure(out)
