"""What progressive JPEG decoding on the device costs, against what a caller pays today and against the sequential twin.
    python tools/jpeg_prog_probe.py [--out profiles/jpeg_prog_probe.json]

For 640x480, 1080p and 4K photograph-like frames (ngx_http_imgproc_amd.workloads.photo_like, quality 90, 4:2:0: what
bench.py's jpeg_pool is made of) written by Pillow as progressive files, as (a) one file, (b) batches of 8 and 64
(a 4K batch of 64 is left out: 1.6 GB of planes), per file:
  device_prog_ms   impgpu_batch_decode_jpeg_ex with IMPGPU_JPEG_PROGRESSIVE, frame complete, and of it the zero fill and
                   level launches (impgpu_jpeg_stage_times [13], [14]) of the call's last group
  host_today_ms    Pillow's decode of the same file on one core + impgpu_image_upload of its pixels
  device_seq_ms    the sequential twin through impgpu_batch_decode_jpeg
Medians of `reps` calls after warm-up; the host clock around the whole call (the calls wait for the device)."""
import ctypes as C
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (first: see tests/conftest.py)
from PIL import Image
import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd.workloads import photo_like


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "jpeg_prog_probe.json")
    torch.set_num_threads(1)
    imp.env_start(0)
    imp.lib.impgpu_jpeg_profile(1)
    out = {"what": __doc__.split("\n")[0], "cases": []}
    for w, h in ((640, 480), (1920, 1080), (3840, 2160)):
        frame = photo_like(h, w, 3)
        files = {}
        for prog in (True, False):
            b = io.BytesIO()
            Image.fromarray(frame).save(b, "JPEG", quality=90, subsampling="4:2:0", progressive=prog)
            files[prog] = b.getvalue()
        for n in (1, 8, 64):
            if n == 64 and w > 1920:
                continue
            reps = 15 if n * w * h < 40e6 else 5
            stage = {}

            def dev_prog():
                res = imp.batch_decode_jpeg_ex([files[True]] * n, imp.JPEG_PROGRESSIVE)
                t = (C.c_double * 16)()
                imp.lib.impgpu_jpeg_stage_times(t, 16)
                stage["levels_us"], stage["level_launches"], stage["files_in_last_group"] = t[13], int(t[14]), int(t[15])
                for rc, im in res:
                    assert rc == 0
                    im.release()

            def dev_seq():
                for rc, im in imp.batch_decode_jpeg([files[False]] * n):
                    assert rc == 0
                    im.release()

            def host_today():
                for _ in range(n):
                    a = np.asarray(Image.open(io.BytesIO(files[True])))
                    im = imp.Image(np.ascontiguousarray(a[:, :, ::-1]))
                    im.release()

            case = dict(width=w, height=h, batch=n, prog_bytes=len(files[True]), seq_bytes=len(files[False]),
                        device_prog_ms=median_ms(dev_prog, reps) / n, host_today_ms=median_ms(host_today, max(3, reps // 3)) / n,
                        device_seq_ms=median_ms(dev_seq, reps) / n)
            case["levels_ms_last_group_per_file"] = stage["levels_us"] / 1e3 / max(1, stage["files_in_last_group"])
            case["level_launches"] = stage["level_launches"]
            out["cases"].append(case)
            print(json.dumps(case), flush=True)
    imp.env_destroy()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
