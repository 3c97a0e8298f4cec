"""Measurements of the device's lossy WebP decoder (impgpu_batch_decode_webp_ex with IMPGPU_WEBP_ACCEPT_LOSSY) against the
route it replaces -- Pillow's libwebp decode of the same file on one core plus impgpu_image_upload of the pixels
-> profiles/webp_lossy_decode_probe.json.

    python tools/webp_lossy_decode_probe.py [--out FILE] [--only GEOMETRY]
                                                     needs the device: per case the time of the device call (host front,
                                                     upload, three launches, the one wait), of the host front alone (a call
                                                     of refused capacity stops behind the parse) and of the host route; the
                                                     files' sizes; whether the frames are Pillow's
    python tools/webp_lossy_decode_probe.py --trace  every case once after a warm-up of each, to be run under
                                                     `rocprofv3 --kernel-trace --output-format csv -- python tools/webp_lossy_decode_probe.py --trace`
    python tools/webp_lossy_decode_probe.py --fold CSV [--out FILE]
                                                     CPU only: the per-kernel times of such a run's kernel_trace.csv into the file

Cases (the lossless table's, tools/webp_decode_probe.py): a lone 640x480 frame, a lone 1920x1080 frame, 64 files of 320x240;
each photo-like, dithered and flat.  The files are Pillow's lossy encodings at quality 75 (method 4, its default).
"""
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from webp_decode_probe import median_ms  # noqa: E402
from webp_encode_probe import GEOMETRIES, KINDS, frames_of  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "webp_lossy_decode_probe.json")
KERNELS = ("k_vp8_dec_recon", "k_vp8_dec_filter", "k_vp8_dec_frame")
ACCEPT = 1                                        # IMPGPU_WEBP_ACCEPT_LOSSY


def files_of(geometry, kind):
    from PIL import Image

    out = []
    for f in frames_of(geometry, kind):
        buf = io.BytesIO()
        Image.fromarray(f[..., [2, 1, 0]]).save(buf, format="WEBP", quality=75)
        out.append(buf.getvalue())
    return out


def pillow_bgr(blob):
    from PIL import Image

    im = Image.open(io.BytesIO(blob))
    im.load()
    return np.asarray(im.convert("RGB"))[..., ::-1]


def cases(only=None):
    return [(g, k) for g in GEOMETRIES for k in KINDS if only in (None, g)]


def measure(out_path, only):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    rows = []
    if only and os.path.exists(out_path):
        with open(out_path) as f:
            rows = [r for r in json.load(f)["rows"] if r["geometry"] != only]
    for g, kind in cases(only):
        blobs = files_of(g, kind)
        big = GEOMETRIES[g][0] >= 1920

        def device():
            res, launches = imp.batch_decode_webp(blobs, accept=ACCEPT)
            for rc, im in res:
                assert rc == 0, rc
                im.release()
            return launches

        def front():
            for b in blobs:
                imp.webp_decode_host(b, capacity=0, guard=0, accept=ACCEPT)

        def host():
            for b in blobs:
                imp.Image(np.ascontiguousarray(pillow_bgr(b))).release()
            imp.sync()

        res, launches = imp.batch_decode_webp(blobs, accept=ACCEPT)
        same = all(rc == 0 and np.array_equal(im.numpy()[..., :3], pillow_bgr(b)) and bool((im.numpy()[..., 3] == 255).all()) for (rc, im), b in zip(res, blobs))
        for _, im in res:
            im.release()
        info = imp.webp_decode_host(blobs[0], capacity=0, guard=0, accept=ACCEPT)[2]
        row = {"geometry": g, "kind": kind, "files": len(blobs), "file_bytes": sum(len(b) for b in blobs), "launches": launches, "frames_equal_pillow": bool(same),
               "feature_word": info[0], "partitions": info[2],
               "device_ms": median_ms(device, 2 if big else 5), "host_front_ms": median_ms(front, 3), "pillow_plus_upload_ms": median_ms(host, 3 if big else 5)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    imp.env_destroy()
    doc = {"what": "impgpu_batch_decode_webp_ex (IMPGPU_WEBP_ACCEPT_LOSSY) against Pillow's decode on one core + impgpu_image_upload; medians, one session",
           "rows": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def trace():
    import torch  # noqa: F401
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    for g, kind in cases():
        blobs = files_of(g, kind)
        for _ in range(2):                                   # a warm-up, then the call the fold reads (the LAST of each case)
            res, _ = imp.batch_decode_webp(blobs, accept=ACCEPT)
            for _, im in res:
                im.release()
    imp.env_destroy()


def fold(csv_path, out_path):
    """the decoder's kernels appear in launch order, two calls a case: the second call's durations, in microseconds"""
    import csv

    with open(csv_path) as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_call = [rows[i:i + 3] for i in range(0, len(rows), 3)]
    assert len(per_call) == 2 * len(cases()), len(per_call)
    with open(out_path) as f:
        doc = json.load(f)
    for k, (g, kind) in enumerate(cases()):
        call = per_call[2 * k + 1]
        split = {[k for k in KERNELS if k in r["Kernel_Name"]][0]: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in call}
        row = [r for r in doc["rows"] if r["geometry"] == g and r["kind"] == kind][0]
        row["kernel_us"] = split
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    if "--trace" in sys.argv:
        trace()
    elif "--fold" in sys.argv:
        fold(sys.argv[sys.argv.index("--fold") + 1], out)
    else:
        measure(out, only)
