#!/usr/bin/env python3
"""Cost of the audio front end (ft8gpu_audio_frames, ft8gpu_decode_audio), measured on the GPU in one session, device pointers:
4096 clips of 15 s int16 audio at 12 kHz, bands (0, 240), on a context of 8192 frames.

  python tools/bench_audio.py [--json profiles/audio_bench.json] [--steps 10] [--rounds 3] [--clips 4096]

The clips: 64 distinct ones, repeated: each 20 CPFSK signals of the bench's message pool at 200 .. 3000 Hz, -18 .. 0 dB in 2500 Hz,
in white noise, synthesised with torch on the GPU.  Three arms, interleaved round by round: the stage, the whole path, and
ft8gpu_decode_messages on the 8192 frames the stage left.  Time = events on the context's stream around `steps` calls, after
three warm-up calls, best of `rounds`; every round's figure is kept.  The stage's algorithmic bytes (the clips in once, the
frames out) over its time are set against the project's measured read-only ceiling of 6.2 .. 6.4 TB/s (profiles/README.md).  The
whole path's records must equal the merge of ft8gpu_decode_messages' records of the stage's frames (checked on the host for the
64 distinct clips).  A machine without a GPU fails at ft8gpu_create; nothing is estimated."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLIPS, DISTINCT, NSIG, BANDS = 4096, 64, 20, (0, 240)
CEILING_TBS = (6.2, 6.4)


def synth_clips(torch, ft8, workload, distinct):
    """int16 [distinct][180000] on the GPU"""
    _, tones = workload.message_pool()
    rng = np.random.default_rng(workload.SEED_BASE)
    n = ft8.AUDIO_NSAMPLES
    sigma = 0.05
    clips = torch.empty((distinct, n), dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(workload.SEED_BASE)
    for c in range(distinct):
        x = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * sigma
        for _ in range(NSIG):
            t = torch.from_numpy(tones[rng.integers(0, len(tones))].astype(np.float64)).cuda()
            f = rng.uniform(200.0, 3000.0) + 6.25 * t.repeat_interleave(1920)
            snr = rng.uniform(-18.0, 0.0)
            amp = np.sqrt(2.0 * sigma ** 2 * 2500.0 / 6000.0 * 10.0 ** (snr / 10.0))
            s0 = int(rng.uniform(0.0, 2.0) * ft8.AUDIO_RATE)
            m = min(f.numel(), n - s0)
            x[s0:s0 + m] += amp * torch.cos(torch.cumsum(2.0 * np.pi * f / ft8.AUDIO_RATE, 0))[:m]
        clips[c] = torch.clamp(torch.round(x * 32768.0), -32768, 32767).to(torch.int16)
    return clips


def merge(msgs, n, bases, message_dtype):
    """the merge rule of include/ft8gpu.h on host arrays: msgs [nclips][nbands][50], n [nclips][nbands]"""
    out = np.zeros((msgs.shape[0], 50 * len(bases)), message_dtype)
    cnt = np.zeros(msgs.shape[0], np.int32)
    for c in range(msgs.shape[0]):
        seen = []
        for b, base in enumerate(bases):
            for k in range(int(n[c, b])):
                rec = msgs[c, b, k].copy()
                key = rec["a91"].tobytes()
                if key in seen:
                    continue
                seen.append(key)
                rec["freq_hz"] = (np.float32(int(rec["cand"]["freq_offset"]) + base) + np.float32(rec["cand"]["freq_sub"]) / np.float32(2)) * np.float32(6.25)
                rec["pad"][0] = b
                out[c, len(seen) - 1] = rec
        cnt[c] = len(seen)
    return out, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=CLIPS)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B, nb = args.clips, len(BANDS)
    distinct = min(DISTINCT, B)
    assert B % distinct == 0
    out = {"what": "cost of the audio front end on one MI355X (tools/bench_audio.py)", "build_id": ft8.check_build_id(), "clips": B,
           "bands": list(BANDS), "frames": B * nb, "format": "S16", "steps": args.steps, "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=B * nb) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        pcm = synth_clips(torch, ft8, workload, distinct).repeat(B // distinct, 1).contiguous()
        iq = torch.empty((B * nb, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")
        msgs, n_msgs = u8(B * nb * 50 * 64), i32(B)                       # the whole path's
        fm, fn = u8(B * nb * 50 * 64), i32(B * nb)                        # ft8gpu_decode_messages' of the stage's frames
        torch.cuda.synchronize()
        arms = {"audio_frames": lambda: dec.audio_frames_dev(pcm, ft8.AUDIO_S16, B, ft8.AUDIO_NSAMPLES, BANDS, iq),
                "decode_audio": lambda: dec.decode_audio_dev(pcm, ft8.AUDIO_S16, B, ft8.AUDIO_NSAMPLES, BANDS, msgs, n_msgs),
                "decode_messages": lambda: dec.decode_messages_dev(iq, B * nb, fm, fn)}
        ms = {name: [] for name in arms}

        def timed(run):
            for _ in range(3):
                run()
            dec.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                run()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / args.steps

        for _ in range(args.rounds):
            for name, run in arms.items():
                ms[name].append(timed(run))
        dec.synchronize()
        for name in arms:
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        stage = out["arms"]["audio_frames"]["best_ms"]
        bytes_in, bytes_out = B * ft8.AUDIO_NSAMPLES * 2, B * nb * 2 * ft8.NSAMPLES * 4
        out["stage_bytes"] = {"in": bytes_in, "out": bytes_out}
        out["stage_tb_per_s"] = round((bytes_in + bytes_out) / (stage * 1e-3) / 1e12, 3)
        out["read_only_ceiling_tb_per_s"] = list(CEILING_TBS)
        out["stage_fraction_of_ceiling"] = round(out["stage_tb_per_s"] / CEILING_TBS[0], 3)
        # 160 products and adds per output and band beside 4.3 bytes moved: the arithmetic, not the memory, sets the time
        out["stage_flop_per_s"] = round(B * nb * ft8.NSAMPLES * 160 / (stage * 1e-3) / 1e12, 3)
        out["stage_bound"] = "bandwidth" if out["stage_fraction_of_ceiling"] >= 0.7 else "VALU"
        out["front_end_share_of_decode_audio"] = round(stage / out["arms"]["decode_audio"]["best_ms"], 4)
        out["messages"] = int(n_msgs.sum().item())
        # the whole path against the merge of the stage's frames' records, on the distinct clips
        d = distinct
        hm = fm.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, nb, 50)[:d]
        hn = fn.cpu().numpy().reshape(B, nb)[:d]
        want_m, want_n = merge(hm, hn, BANDS, ft8.MESSAGE_DTYPE)
        got_m = msgs.cpu().numpy().view(ft8.MESSAGE_DTYPE).reshape(B, 50 * nb)[:d]
        got_n = n_msgs.cpu().numpy()[:d]
        same = bool((got_n == want_n).all()) and all(got_m[c, :want_n[c]].tobytes() == want_m[c, :want_n[c]].tobytes() for c in range(d))
        out["records_equal_merge_of_decode_messages"] = same
        out["repeats_equal"] = bool(torch.equal(n_msgs[:d], n_msgs[B - d:]))
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0 if out["records_equal_merge_of_decode_messages"] and out["repeats_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
