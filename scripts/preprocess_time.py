#!/usr/bin/env python3
"""Frame preprocessing of one clip, device path against host path: 16 decoded 720x1280 uint8 frames with
max_image_size = 320 (BOX -> 640x360, BICUBIC -> 320x180, crop -> 176x320, normalise; the shapes of the scripted inference
run), through LVMProcessor.process_frames (csrc/preprocess.hip) and through process_image on PIL images.

One process.  The device leg starts from frames already on the GPU and a warm table cache and workspace; it is timed with
device events around REPS calls, ROUNDS times, alternating with the host leg, which is timed with the host clock: Pillow
alone (PIL images in, CPU tensors out), and with the copies a user whose frames live on the GPU pays around it (frames to
the host, result back).  The outputs of the two legs are compared with torch.equal first.  `bytes` is what the four
launches must read and write, computed from the plan's shapes (tables excluded); its rate is set against 8 TB/s of HBM.

The parent starts the measurement as a child process under a time limit of its own and never touches the GPU itself.  One
JSON line per result, to stdout and to the log:
    timeout -k 10 300 python3 scripts/preprocess_time.py [--out profiles/preprocess_time.log]
"""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 240
N, H, W, MAX_SIZE = 16, 720, 1280, 320
REPS, ROUNDS = 50, 5
HBM_PEAK = 8.0e12


def plan_bytes(steps, box, n, h, w):
    """Bytes the passes of a plan read and write: every resize is a horizontal pass (if the width changes) and a vertical
    one (if the height changes); the last vertical pass reads only the crop's columns and writes fp32 planes."""
    total, launches = 0, 0
    for i, (_, (sw, sh)) in enumerate(steps):
        last = i == len(steps) - 1
        if sw != w:
            total += n * h * (w + sw) * 3
            launches += 1
            w = sw
        if sh != h:
            if last:
                total += n * h * (box[2] - box[0]) * 3 + n * 3 * (box[3] - box[1]) * (box[2] - box[0]) * 4
            else:
                total += n * (h + sh) * w * 3
            launches += 1
            h = sh
        elif last:
            total += n * (box[3] - box[1]) * (box[2] - box[0]) * (3 + 12)
            launches += 1
    return total, launches


def child(out_path):
    import numpy as np
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_time.py needs a GPU")
    P = importlib.import_module("video-gpt_amd.processor")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    log = open(out_path, "w")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    dev = torch.device("cuda:0")
    proc = P.LVMProcessor(P.SpecialTokenizer(10, 11, 12), max_image_size=MAX_SIZE)
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    base = (127 + 100 * np.sin(xx / 37.0) * np.cos(yy / 23.0))[None, :, :, None]
    frames = np.clip(base + rng.normal(0, 30, (N, H, W, 3)), 0, 255).astype(np.uint8)
    pil = [Image.fromarray(f) for f in frames]
    xd = torch.from_numpy(frames).to(dev)
    steps, box = P.crop_arr_plan(W, H, MAX_SIZE)
    nbytes, launches = plan_bytes(steps, box, N, H, W)

    want = torch.stack([proc.process_image(im) for im in pil])
    got = proc.process_frames(xd)
    torch.cuda.synchronize()
    emit(workload=f"{N} x {H}x{W} -> {tuple(got.shape)}", plan=[[f, list(s)] for f, s in steps], crop_box=list(box),
         pillow=Image.__version__, equal_to_host_path=bool(torch.equal(got.cpu(), want)), launches=launches, bytes=nbytes)

    def device_leg():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            proc.process_frames(xd)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / REPS

    def host_leg(round_trip):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if round_trip:
            imgs = [Image.fromarray(f) for f in xd.cpu().numpy()]
        else:
            imgs = pil
        out = torch.stack([proc.process_image(im) for im in imgs])
        if round_trip:
            out = out.to(dev)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    device_leg(), host_leg(False), host_leg(True)   # warm-up of every leg
    ms = {"device": [], "host_pillow": [], "host_round_trip": []}
    for _ in range(ROUNDS):
        ms["device"].append(round(device_leg(), 4))
        ms["host_pillow"].append(round(host_leg(False), 2))
        ms["host_round_trip"].append(round(host_leg(True), 2))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    rate = nbytes / (med["device"] * 1e-3)
    emit(ms_per_clip=ms, median_ms=med, device_call_is=f"mean of {REPS} calls per event window",
         device_TB_s=round(rate / 1e12, 3), of_8_TB_s=round(rate / HBM_PEAK, 4),
         host_pillow_over_device=round(med["host_pillow"] / med["device"], 1),
         host_round_trip_over_device=round(med["host_round_trip"] / med["device"], 1))
    log.close()


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "preprocess_time.log")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    if "--child" in args:
        child(out)
    else:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", out], timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"preprocess_time.py: the measurement did not finish within {LIMIT_S} s")
        sys.exit(rc)
