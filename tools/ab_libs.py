#!/usr/bin/env python3
"""A/B of two (or more) BUILDS of libft8gpu.so in ONE process and GPU session -- boxes of the pool differ by several
percent, so only arms that share a box and a session are comparable.  Every arm decodes the same batch; arms are
interleaved round by round; the records of all arms must be byte-identical.
  python tools/ab_libs.py --libs tools/ab/libft8gpu_prev.so rtlsdr_ft8d_amd/libft8gpu.so [--config 2|4] [--rounds 3] [--entry batch|messages]
--entry messages times ft8gpu_decode_messages (64-byte records of every message) instead of ft8gpu_decode_batch; --entry
subtracted times ft8gpu_decode_messages_subtracted at three passes (records, counts and the counts by pass in the digest);
--entry demod / demod_stage time ft8gpu_decode_messages_demod / ft8gpu_demod_candidates at 48 candidates per frame (the counts by
stage, or the status and info records, in the digest).  A library may be named more than once (parent this this parent)."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", required=True)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--config", type=int, default=2, choices=(2, 4))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--entry", choices=("batch", "messages", "subtracted", "demod", "demod_stage"), default="batch")
    ap.add_argument("--torch-stream", action="store_true", help="run every arm on a torch.cuda.Stream (as bench.py does) instead of the context's own stream")
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    cfg = {2: dict(frames=4096, nsig=20, snr=(-18.0, 0.0), maxc=120), 4: dict(frames=1024, nsig=60, snr=(-24.0, -14.0), maxc=480)}[args.config]
    B = args.frames or cfg["frames"]
    libs = [ft8.load_library() if os.path.abspath(p) == ft8.LIB_PATH else ft8.load_library_at(p) for p in args.libs]
    decs = [ft8.Decoder(device=0, max_frames=B, max_candidates=cfg["maxc"], lib=L) for L in libs]
    if args.torch_stream:
        ts = torch.cuda.Stream()
        torch.cuda.set_stream(ts)
        for d in decs:
            d.set_stream(ts.cuda_stream)
    _, tones = workload.message_pool()
    sig, _ = workload.frame_signals(0, B, cfg["nsig"], tones, snr_range=cfg["snr"])
    iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
    decs[0].synth_frames(sig, B, cfg["nsig"], 1.0, workload.SEED_BASE, iq)
    spots = torch.zeros((B, 1400 if args.entry == "batch" else 50 * 64), dtype=torch.uint8, device="cuda")
    nres = torch.zeros((B,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    res = [{"lib": p, "ms": [], "stages": None, "digest": None} for p in args.libs]
    nbp = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
    extra = []                                # further outputs that go into the digest
    if args.entry in ("demod", "demod_stage"):
        # the demodulation from the I/Q samples at its recommended values, 48 candidates per frame: the whole path, or the stage
        # alone on the first arm's BP status records
        maxc = cfg["maxc"]
        if args.entry == "demod_stage":
            u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
            mag, cands, status, status2, info = u8(B * ft8.MAG_ARRAY), u8(B * maxc * 8), u8(B * maxc * 48), u8(B * maxc * 48), u8(B * maxc * 16)
            decs[0].waterfall_dev(iq, B, mag)
            decs[0].find_sync_dev(mag, B, cands, nres)
            decs[0].decode_candidates_dev(mag, cands, nres, B, status)
            decs[0].synchronize()
            extra = [status2, info]
        else:
            extra = [torch.zeros((B, 2), dtype=torch.int32, device="cuda")]
    run = {"batch": lambda d: d.decode_batch_dev(iq, B, spots, nres), "messages": lambda d: d.decode_messages_dev(iq, B, spots, nres),
           "subtracted": lambda d: d.decode_messages_subtracted_dev(iq, B, 3, spots, nres, nbp),
           "demod": lambda d: d.decode_messages_demod_dev(iq, B, ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS, 48, spots, nres, extra[0]),
           "demod_stage": lambda d: d.demod_candidates_dev(iq, cands, nres, status, B, ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS, 48,
                                                           status2, info)}[args.entry]
    for _ in range(args.rounds):
        for dec, r in zip(decs, res):
            for _ in range(3):
                run(dec)
            dec.synchronize()
            dec.enable_timing(True)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(dec)
            r.setdefault("host_enqueue_ms", []).append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            dec.synchronize()
            r["ms"].append(round(1e3 * (time.perf_counter() - t0) / args.steps, 4))
            if args.entry != "demod_stage":                            # a stage entry records no pipeline run
                st = dec.timings()
                r["stages"] = {k: round(v, 4) for k, v in st.items() if k.endswith("_ms")}
            dec.enable_timing(False)
            r["digest"] = hashlib.sha256(spots.cpu().numpy().tobytes() + nres.cpu().numpy().tobytes() +
                                         (nbp.cpu().numpy().tobytes() if args.entry == "subtracted" else b"") +
                                         b"".join(t.cpu().numpy().tobytes() for t in extra)).hexdigest()[:16]
    for r in res:
        r["best_ms"] = min(r["ms"])
    out = {"frames": B, "config": args.config, "entry": args.entry, "steps": args.steps, "arms": res,
           "all_digests_equal": len({r["digest"] for r in res}) == 1}
    for d in decs:
        d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
