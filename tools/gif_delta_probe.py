"""GIF answers with delta frames (IMPGPU_GIF_ENC_DELTA) against the same call without the bit, in one session on the same
albums, flag off and on alternating:

    8x640x480_exact        an 8-frame 640 x 480 album: a still dithered background of 200 colours, a 64 x 64 patch that moves
    8x640x480_blurred      the same over photo content (past 256 colours), under IMPGPU_GIF_ENC_QUANTIZE
    64x8x320x240_exact     64 albums of 8 frames at 320 x 240 of the first kind
    64x8x320x240_blurred   ... and of the second
    8x640x480_all_change   every pixel of every frame changes: the bit's worst case, which pays k_gif_enc_delta and the second
                           colour set and gains nothing

Times are wall time of the call, medians over --iters calls after a warm-up call, in ms, in two halves (off, on, on, off);
"file_bytes" are the files of all the call's albums.  The flagged files are checked against the host twin's.

--unflagged-only: the calls without the bit alone, through the _ex entry points -- what a checkout of the parent commit can
run too (--package-root names its tree): the rows that show the unflagged route moved only within run-to-run spread.

--fold LABEL=FILE ... : no device is touched; the rows of such --unflagged-only runs go into --out (which exists) as
"unflagged_route_same_session".

    timeout -k 10 600 python tools/gif_delta_probe.py [--iters 9] [--out profiles/gif_delta_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # noqa: F401  (first: the HIP runtime torch bundles, as in bench.py)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("8x640x480_exact", 640, 480, 8, 1, "exact"), ("8x640x480_blurred", 640, 480, 8, 1, "blurred"),
         ("64x8x320x240_exact", 320, 240, 8, 64, "exact"), ("64x8x320x240_blurred", 320, 240, 8, 64, "blurred"),
         ("8x640x480_all_change", 640, 480, 8, 1, "all_change")]


def photo():
    from PIL import Image

    return np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "jpeg", "c420_q50_640x480.jpg")).convert("RGB"))[..., ::-1]


def album(base, w, h, frames, kind, seed):
    """BGRA frames: a background (dithered 200 colours, or the photo) and a 64 x 64 patch of a ramp at a place per frame"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (200, 3)).astype(np.uint8)
    if kind == "blurred":
        back = base[:: 480 // h, :: 640 // w][:h, :w].astype(np.uint8)
    else:
        back = pal[rng.integers(0, 200, (h, w))]
    yy, xx = np.mgrid[0:64, 0:64]
    out = []
    for f in range(frames):
        g = pal[rng.integers(0, 200, (h, w))] if kind == "all_change" else back.copy()
        x0, y0 = (f * 61) % (w - 64), (f * 37) % (h - 64)
        patch = np.stack([xx * 4, yy * 4, np.full_like(xx, 30 * f)], 2).astype(np.uint8) if kind == "blurred" else pal[(xx // 8 + yy // 8 + f) % 200]
        g[y0:y0 + 64, x0:x0 + 64] = patch
        out.append(np.ascontiguousarray(np.concatenate([g, np.full((h, w, 1), 255, np.uint8)], 2)))
    return out


def median_ms(fn, iters):
    fn()
    ts = []
    for _ in range(max(1, iters)):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def fold(out, runs):
    result = json.load(open(out))
    block = {"what": "tools/gif_delta_probe.py --iters 9 --unflagged-only (impgpu_batch_encode_gif_ex, flags 0 or IMPGPU_GIF_ENC_QUANTIZE), three "
                     "processes one after the other on one device, ahead of the rows above; the parent commit's package through --package-root",
             "runs": {}}
    for item in runs:
        label, path = item.split("=", 1)
        block["runs"][label] = {r["case"]: {"flags": r["flags_off"], "launches": r["off_launches"], "file_bytes": r["off_file_bytes"], "ms": r["off_ms"],
                                            "halves_ms": r["off_halves_ms"]} for r in json.load(open(path))["rows"]}
    result["unflagged_route_same_session"] = block
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--unflagged-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--label", default="")
    ap.add_argument("--fold", nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_delta_probe.json"))
    a = ap.parse_args()
    if a.fold:
        fold(a.out, a.fold)
        return
    sys.path.insert(0, os.path.abspath(a.package_root))
    import ngx_http_imgproc_amd as imp

    imp.env_start(0)
    base = photo()
    rows = []
    for name, w, h, frames, albums, kind in CASES:
        if a.only and a.only != name:
            continue
        quant = imp.GIF_ENC_QUANTIZE if kind == "blurred" else 0
        host_frames = [album(base, w, h, frames, kind, 7 + k) for k in range(min(albums, 4))]
        host_frames = [host_frames[k % len(host_frames)] for k in range(albums)]
        images = [imp.Image.album(fr) for fr in host_frames]
        n = albums
        handles = (C.c_void_p * n)(*[im.h.value for im in images])
        bound = imp.gif_encode_bound(w, h, frames)
        bufs = [np.empty(bound, np.uint8) for _ in range(n)]
        outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        caps, lens, codes, launches = (C.c_size_t * n)(*[bound] * n), (C.c_size_t * n)(), (C.c_int * n)(), C.c_int()
        loops = (C.c_int * n)(*[0] * n)

        def off():
            rc = imp.lib.impgpu_batch_encode_gif_ex(handles, None, None, loops, n, a.segment, quant, outs, caps, lens, codes, C.byref(launches))
            assert rc == 0 and not any(codes), (rc, list(codes))

        def on():
            rc = imp.lib.impgpu_batch_encode_gif_ex2(handles, None, None, loops, n, a.segment, quant | imp.GIF_ENC_DELTA, outs, caps, lens, codes,
                                                     C.byref(launches))
            assert rc == 0 and not any(codes), (rc, list(codes))

        h1, h2 = a.iters // 2, a.iters - a.iters // 2
        row = {"probe": "gif_delta", "case": name, "canvas": [w, h], "frames": frames, "albums": albums, "iters": a.iters,
               "segment": a.segment or imp.GIF_ENC_SEGMENT, "flags_off": quant}
        if a.label:
            row["build"] = a.label
        off()
        row["off_file_bytes"], row["off_launches"] = int(sum(lens)), launches.value
        if a.unflagged_only:
            o1, o2 = median_ms(off, h1), median_ms(off, h2)
        else:
            on()
            row["on_file_bytes"], row["on_launches"] = int(sum(lens)), launches.value
            for k in range(min(n, 2)):                               # the files are the host twin's, byte for byte
                rc, blob, m, _ = imp.encode_gif_host(host_frames[k], loop_count=0, segment=a.segment, flags=quant, delta=True)
                assert rc == 0 and bufs[k][: lens[k]].tobytes() == blob
            o1, n1 = median_ms(off, h1), median_ms(on, h1)
            n2, o2 = median_ms(on, h2), median_ms(off, h2)
            row.update({"flags_on": quant | imp.GIF_ENC_DELTA, "on_ms": round((n1 + n2) / 2, 3), "on_halves_ms": [round(n1, 3), round(n2, 3)],
                        "on_over_off_ms": round((n1 + n2) / (o1 + o2), 3), "on_over_off_bytes": round(row["on_file_bytes"] / row["off_file_bytes"], 4)})
        row.update({"off_ms": round((o1 + o2) / 2, 3), "off_halves_ms": [round(o1, 3), round(o2, 3)]})
        rows.append(row)
        print(json.dumps(row), flush=True)
        for im in images:
            im.release()
    imp.env_destroy()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
