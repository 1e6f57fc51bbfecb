#!/usr/bin/env python3
"""A/B of builds of libft8gpu.so on the RX front end (ft8gpu_rx_decimate, device pointers): interleaved rounds in one
process, outputs must be bit-identical.   python tools/ab_rx.py --libs a.so b.so [--captures 16] [--rounds 4]
--stream 16x1 4x4 adds arms that run ft8gpu_rx_stream of the LAST library on the same raw bytes cut into
STREAMSxSLOTS (the state is carried from call to call while timing, as a daemon would; the digest is taken from one
more call from the reset state, and for Nx1 it must equal ft8gpu_rx_decimate's)."""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--captures", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--stream", nargs="*", default=[], metavar="STREAMSxSLOTS")
    ap.add_argument("--json", help="also write the result there")
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    npairs = 36_000_000
    libs = [ft8.load_library() if os.path.abspath(p) == ft8.LIB_PATH else ft8.load_library_at(p) for p in args.libs]
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    decs = [ft8.Decoder(device=0, max_frames=args.captures, lib=L) for L in libs]
    for d in decs:
        d.set_stream(stream.cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (args.captures, 2 * npairs), dtype=torch.uint8, device="cuda", generator=g)
    iq = torch.empty((args.captures, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
    res = [{"lib": p, "build_id": ft8.build_id(L), "entry": "ft8gpu_rx_decimate", "ms": [], "digest": None} for p, L in zip(args.libs, libs)]
    shapes = [tuple(map(int, t.split("x"))) for t in args.stream]
    assert all(a * b == args.captures for a, b in shapes), "STREAMS x SLOTS must equal --captures (the same raw bytes)"
    sres = [{"lib": args.libs[-1], "build_id": ft8.build_id(libs[-1]), "entry": "ft8gpu_rx_stream", "streams": a, "slots": b, "ms": [], "digest": None}
            for a, b in shapes]
    state = torch.zeros((args.captures, 516), dtype=torch.uint8, device="cuda")
    n_out = torch.empty(args.captures, dtype=torch.int32, device="cuda")
    for _ in range(args.rounds):
        for (a, b), r in zip(shapes, sres):
            dec = decs[-1]
            state.zero_()
            for _ in range(3):
                dec.rx_stream_dev(raw, a, b, npairs, state, iq, n_out, True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                dec.rx_stream_dev(raw, a, b, npairs, state, iq, n_out, True)
            e1.record(stream)
            torch.cuda.synchronize()
            r["ms"].append(round(e0.elapsed_time(e1) / args.steps, 4))
            state.zero_()
            dec.rx_stream_dev(raw, a, b, npairs, state, iq, n_out, True)
            torch.cuda.synchronize()
            r["digest"] = hashlib.sha256(iq.cpu().numpy().tobytes()).hexdigest()[:16]
        for dec, r in zip(decs, res):
            for _ in range(3):
                dec.rx_decimate_dev(raw, args.captures, npairs, iq, True)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                dec.rx_decimate_dev(raw, args.captures, npairs, iq, True)
            e1.record(stream)
            torch.cuda.synchronize()
            r["ms"].append(round(e0.elapsed_time(e1) / args.steps, 4))
            r["digest"] = hashlib.sha256(iq.cpu().numpy().tobytes()).hexdigest()[:16]
    for r in res + sres:
        r["ms_median"] = sorted(r["ms"])[len(r["ms"]) // 2]
    out = {"captures": args.captures, "npairs": npairs, "steps": args.steps, "arms": res + sres,
           "all_digests_equal": len({r["digest"] for r in res}) == 1,
           "stream_from_reset_equals_decimate": all(r["digest"] == res[-1]["digest"] for r in sres if r["slots"] == 1)}
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
