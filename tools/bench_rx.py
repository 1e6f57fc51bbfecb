#!/usr/bin/env python3
"""Throughput of the RX front end (rtlsdr_callback(), rtlsdr_ft8d.c:76-202) on
one MI355X: raw 2.4 Msps unsigned 8-bit I/Q captures resident in HBM -> decimated, normalised 15 s frames.
Not the BASELINE metric (bench.py reports that); this is the HBM-bound neighbour of the hot path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cpu-captures", type=int, default=1)
    ap.add_argument("--stream", metavar="STREAMSxSLOTS", help="time ft8gpu_rx_stream (filter state carried from slot to slot and from "
                    "call to call) on the same raw bytes cut into STREAMS x SLOTS = --captures; the CPU check then chains the oracle")
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    npairs = 36_000_000                       # 15 s at 2.4 Msps
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    dec = ft8.Decoder(device=0, max_frames=args.captures)
    dec.set_stream(stream.cuda_stream)
    g = torch.Generator(device=dev).manual_seed(1)
    raw = torch.randint(0, 256, (args.captures, 2 * npairs), dtype=torch.uint8, device=dev, generator=g)
    iq = torch.empty((args.captures, 2, ft8.NSAMPLES), dtype=torch.float32, device=dev)
    if args.stream:
        nstreams, nslots = map(int, args.stream.split("x"))
        assert nstreams * nslots == args.captures, "STREAMS x SLOTS must equal --captures"
        state = torch.zeros((nstreams, 516), dtype=torch.uint8, device=dev)
        run = lambda: dec.rx_stream_dev(raw, nstreams, nslots, npairs, state, iq, None, True)
    else:
        run = lambda: dec.rx_decimate_dev(raw, args.captures, npairs, iq, True)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.steps):
        run()
    e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    bytes_in = args.captures * 2 * npairs
    bytes_out = args.captures * 2 * ft8.NSAMPLES * 4
    out = {"stage": "rx front end (rtlsdr_callback)" + (f", state carried, {args.stream} streams x slots" if args.stream else ""), "captures_per_launch": args.captures, "ms_per_launch": round(ms, 3),
           "captures_per_s": round(args.captures / ms * 1e3, 1),
           "roofline": {"bound": "hbm", "achieved": round((bytes_in + bytes_out) / ms / 1e6, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round((bytes_in + bytes_out) / ms / 1e6 / 8000.0, 4),
                        "algorithmic_bytes_per_launch": bytes_in + bytes_out, "traffic": None}}
    try:        # HBM bytes of the block kernel from the committed counter passes (16 captures per launch), scaled to this launch
        with open(os.path.join(ROOT, "profiles", "r04_rx_pmc_traffic.json")) as f:
            pm = json.load(f)["block_kernel"]
        out["roofline"]["traffic"] = int((pm["fetch_bytes_per_launch_corrected"] + pm["write_bytes_per_launch_raw"]) * args.captures / 16)
        out["roofline"]["traffic_from"] = "profiles/r04_rx_pmc_traffic.json (block kernel: FETCH_SIZE x 2 + WRITE_SIZE, per 16 captures)"
    except (OSError, KeyError, ValueError):
        pass
    if args.cpu_captures > 0:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        if args.stream:                         # one more call from the reset state: the first slots of stream 0 against the oracle chain
            state.zero_()
            run()
            torch.cuda.synchronize()
            args.cpu_captures = min(args.cpu_captures, nslots)
        h = raw[:args.cpu_captures].cpu().numpy()
        t0 = time.perf_counter()
        ok = 0
        g_iq = iq[:args.cpu_captures].cpu().numpy()
        if args.stream:
            import rx_stream_util
            want, _, _ = rx_stream_util.oracle_chain(h, None, True)
            ok = sum(int(np.array_equal(want[k].view(np.uint32), g_iq[k].view(np.uint32))) for k in range(args.cpu_captures))
        for k in range(0 if args.stream else args.cpu_captures):
            i, q, _ = oracle_lib.rx_capture(h[k], normalise=True)
            ok += int(np.array_equal(i, g_iq[k, 0]) and np.array_equal(q, g_iq[k, 1]))
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(args.cpu_captures / dt, 3), "unit": "captures/s", "cores": 1, "kind": "port",
                               "sample": f"{args.cpu_captures} capture(s) through oracle " + ("ft8o_rx_callback, state carried" if args.stream else "ft8o_rx_capture"), "identical": f"{ok}/{args.cpu_captures}"}
    dec.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
