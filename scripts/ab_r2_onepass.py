#!/usr/bin/env python3
"""A/B of k_reduce2x2's two bodies in one process: the chunk-loop tile (MIPX_R2_VARIANT=578,
the body shipped before) against the one-pass tile (the default, variant 66).

C2 (256 x 3840x2160x3) and 4K RGBA at the largest batch that fits in 90 % of the free
device memory (at most 1024 images, which keeps an arm's round near a second).  The arms
alternate, ROUNDS (default 7) rounds of 20 warm-up + 100 timed steps each, HIP events
around the timed steps.  Both arms are checked against the oracle once.  Every round is a
line of the record (default profiles/r08/r2_onepass_ab.jsonl), then one summary line per
configuration: the new arm counts as faster only if its slowest round beats the old
arm's fastest, and as slower only if its fastest round loses to the old arm's slowest.

    python scripts/ab_r2_onepass.py [--out FILE] [--rounds N]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from imaginary_amd._abi import check, lib  # noqa: E402
from oracle import oracle as o  # noqa: E402

W, H = 3840, 2160
ARMS = (("loop578", "578"), ("onepass66", ""))
WARMUP, STEPS = 20, 100


def select(variant):
    os.environ.pop("MIPX_R2_BAND", None)
    if variant:
        os.environ["MIPX_R2_VARIANT"] = variant
    else:
        os.environ.pop("MIPX_R2_VARIANT", None)
    lib.mipx_tuning_reload()  # the library snapshots the MIPX_* knobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "r2_onepass_ab.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 rounds"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda", 0)
    lib.mipx_set_device(0)
    check(lib.mipx_set_reduce_sampling(0), "corner sampling")
    o.build()
    o.set_switch("reduce_centre", 0)
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        out.write(line + "\n")
        out.flush()
        print(line, flush=True)

    for name, b, n in (("C2_rgb", 3, 256), ("4k_rgba", 4, None)):
        per_img = H * W * b + (H // 2) * (W // 2) * b
        if n is None:
            free, _total = torch.cuda.mem_get_info(dev)
            n = max(1, min(1024, int(0.9 * free) // per_img))
        x = torch.randint(0, 256, (n, H, W, b), dtype=torch.uint8, device=dev)
        y = torch.empty((n, H // 2, W // 2, b), dtype=torch.uint8, device=dev)

        def step():
            check(lib.mipx_op_reduce(x.data_ptr(), y.data_ptr(), n, W, H, b, 2.0, 2.0, None, 0, sp), "reduce")

        probe = sorted({0, n - 1})
        want = {i: o.reduce(x[i].cpu().numpy(), 2.0, 2.0) for i in probe}
        for arm, variant in ARMS:
            select(variant)
            y.fill_(0xA5)
            step()
            torch.cuda.synchronize()
            ok = all(np.array_equal(y[i].cpu().numpy(), want[i]) for i in probe)
            emit({"config": name, "arm": arm, "batch": n, "verified_vs_oracle": ok, "images_checked": probe})
            assert ok, f"{name} {arm} differs from the oracle"
        times = {arm: [] for arm, _ in ARMS}
        for rnd in range(args.rounds):
            for arm, variant in ARMS:
                select(variant)
                for _ in range(WARMUP):
                    step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(STEPS):
                    step()
                e1.record(st)
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / STEPS
                times[arm].append(ms)
                emit({"config": name, "round": rnd, "arm": arm, "batch": n, "ms_per_step": round(ms, 5),
                      "tb_per_s": round(n * per_img / ms / 1e9, 4)})
        old, new = times[ARMS[0][0]], times[ARMS[1][0]]
        verdict = "faster" if max(new) < min(old) else "slower" if min(new) > max(old) else "within spread"
        emit({"config": name, "summary": True, "batch": n, "rounds": args.rounds,
              "loop578_ms": {"min": round(min(old), 5), "median": round(float(np.median(old)), 5),
                             "max": round(max(old), 5)},
              "onepass66_ms": {"min": round(min(new), 5), "median": round(float(np.median(new)), 5),
                               "max": round(max(new), 5)},
              "onepass_vs_loop_median": round(float(np.median(new) / np.median(old)), 4), "onepass_is": verdict})
        del x, y
        torch.cuda.empty_cache()
    select("")
    out.close()


if __name__ == "__main__":
    main()
