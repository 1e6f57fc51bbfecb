#!/usr/bin/env python3
"""Cost of a-priori decoding on the demodulated soft bits (ft8gpu_demod_soft, ft8gpu_ap_soft_candidates,
ft8gpu_decode_messages_demod_ap), measured on the GPU in one session, device pointers, on 4096 frames of the bench workload
(20 signals, -18 .. 0 dB, cap 120).

  python tools/bench_demod_ap.py [--json profiles/demod_ap_bench.json] [--steps 5] [--rounds 3]

Arms, interleaved round by round: the demodulation stage without and with the soft bits written out (ft8gpu_demod_candidates /
ft8gpu_demod_soft) at max_per_frame = 16, 48 and the cap; ft8gpu_ap_soft_candidates at 1 and 4 hypotheses on the array and the
status records the emitting stage left at the cap, beside ft8gpu_ap_candidates at 1 and 4 hypotheses on the same batch's BP status
records; ft8gpu_decode_messages_demod beside ft8gpu_decode_messages_demod_ap ("CQ ? ?").  Time = events on the context's stream
around `steps` calls, after two warm-up calls, best of `rounds`; every round's figure is kept.  The records and the first two
count columns of the whole path must equal ft8gpu_decode_messages_demod's.  A machine without a GPU fails at ft8gpu_create;
nothing is estimated."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES, CAP = 4096, 120
FOUR = ("CQ ? ?", "CQ DX ? ?", "K1ABC ? ?", "CQ POTA ? ?")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=FRAMES)
    args = ap.parse_args()
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    B = args.frames
    SETS, GATE, APGATE = ft8.DEMOD_SETS, ft8.DEMOD_MAX_HARD_ERRORS, ft8.APSOFT_MAX_HARD_ERRORS
    out = {"what": "cost of a-priori decoding on the demodulated soft bits on one MI355X (tools/bench_demod_ap.py)",
           "build_id": ft8.check_build_id(), "frames": B, "max_candidates": CAP, "sets": SETS, "max_hard_errors": GATE,
           "ap_max_hard_errors": APGATE, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    with ft8.Decoder(device=0, max_frames=B, max_candidates=CAP) as dec:
        stream = torch.cuda.ExternalStream(dec.stream_handle())
        _, tones = workload.message_pool()
        sig, _ = workload.frame_signals(0, B, 20, tones, snr_range=(-18.0, 0.0))
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device="cuda")
        dec.synth_frames(sig, B, 20, 1.0, workload.SEED_BASE, iq)
        u8 = lambda n: torch.zeros((n,), dtype=torch.uint8, device="cuda")
        i32 = lambda n: torch.zeros((n,), dtype=torch.int32, device="cuda")
        mag, cands, status, counts = u8(B * ft8.MAG_ARRAY), u8(B * CAP * 8), u8(B * CAP * 48), i32(B)
        status2, info, status3, ainfo, apinfo = u8(B * CAP * 48), u8(B * CAP * 16), u8(B * CAP * 48), u8(B * CAP * 20), u8(B * CAP * 8)
        soft = torch.zeros((B * CAP * 3 * ft8.SOFT_STRIDE,), dtype=torch.float32, device="cuda")
        msgs, n_msgs, nbs = u8(B * 50 * 64), i32(B), i32(2 * B)
        msgs2, n_msgs2, nbs3 = u8(B * 50 * 64), i32(B), i32(3 * B)
        dec.waterfall_dev(iq, B, mag)
        dec.find_sync_dev(mag, B, cands, counts)
        dec.decode_candidates_dev(mag, cands, counts, B, status)
        dec.demod_soft_dev(iq, cands, counts, status, B, SETS, GATE, CAP, status2, info, soft)
        dec.synchronize()
        cnt = counts.cpu().numpy()
        live = (torch.arange(CAP)[None, :].numpy() < cnt[:, None])

        def failing(t):
            st = t.cpu().numpy().view(ft8.STATUS_DTYPE).reshape(B, CAP)
            return int((live & (st["ok"] == 0) & (st["ldpc_errors"] != 0)).sum())

        out["candidates"], out["failing_after_bp"], out["failing_after_demod"] = int(cnt.sum()), failing(status), failing(status2)
        stage = lambda mpf: (lambda: dec.demod_candidates_dev(iq, cands, counts, status, B, SETS, GATE, mpf, status3, info))
        emit = lambda mpf: (lambda: dec.demod_soft_dev(iq, cands, counts, status, B, SETS, GATE, mpf, status3, info, soft))
        arms = {}
        for mpf in (16, 48, CAP):
            arms["demod_candidates_mpf%d" % mpf] = stage(mpf)
            arms["demod_soft_mpf%d" % mpf] = emit(mpf)                # the cap comes last: soft is the array of the cap again for the AP arms
        arms.update({
            "ap_soft_h1": lambda: dec.ap_soft_candidates_dev(soft, counts, status2, B, SETS, FOUR[:1], APGATE, status3, ainfo),
            "ap_soft_h4": lambda: dec.ap_soft_candidates_dev(soft, counts, status2, B, SETS, FOUR, APGATE, status3, ainfo),
            "ap_h1": lambda: dec.ap_candidates_dev(mag, cands, counts, status, B, FOUR[:1], ft8.AP_MAX_HARD_ERRORS, status3, apinfo),
            "ap_h4": lambda: dec.ap_candidates_dev(mag, cands, counts, status, B, FOUR, ft8.AP_MAX_HARD_ERRORS, status3, apinfo),
            "decode_messages_demod": lambda: dec.decode_messages_demod_dev(iq, B, SETS, GATE, CAP, msgs, n_msgs, nbs),
            "decode_messages_demod_ap": lambda: dec.decode_messages_demod_ap_dev(iq, B, SETS, GATE, CAP, FOUR[:1], APGATE, msgs2, n_msgs2, nbs3)})
        ms = {name: [] for name in arms}

        def timed(run):
            for _ in range(2):
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
        for name in arms:
            out["arms"][name] = {"ms": [round(x, 4) for x in ms[name]], "best_ms": round(min(ms[name]), 4)}
        best = lambda name: out["arms"][name]["best_ms"]
        out["emit_over_plain"] = {str(mpf): round(best("demod_soft_mpf%d" % mpf) / best("demod_candidates_mpf%d" % mpf), 4) for mpf in (16, 48, CAP)}
        out["ap_soft_over_ap"] = {"h1": round(best("ap_soft_h1") / best("ap_h1"), 4), "h4": round(best("ap_soft_h4") / best("ap_h4"), 4)}
        out["whole_path_over_demod"] = round(best("decode_messages_demod_ap") / best("decode_messages_demod"), 4)
        # the whole paths once more for the figures
        dec.decode_messages_demod_dev(iq, B, SETS, GATE, CAP, msgs, n_msgs, nbs)
        dec.decode_messages_demod_ap_dev(iq, B, SETS, GATE, CAP, FOUR[:1], APGATE, msgs2, n_msgs2, nbs3)
        dec.synchronize()
        n1, n2 = n_msgs.cpu().numpy(), n_msgs2.cpu().numpy()
        hb, hb3 = nbs.cpu().numpy().reshape(B, 2), nbs3.cpu().numpy().reshape(B, 3)
        a, b = msgs.cpu().numpy().reshape(B, 50, 64), msgs2.cpu().numpy().reshape(B, 50, 64)
        out["records_equal_decode_messages_demod"] = bool((hb3[:, :2] == hb).all() and (hb3[:, 2] == n2).all() and
                                                          all(a[f, :n1[f]].tobytes() == b[f, :n1[f]].tobytes() for f in range(B)))
        out["messages_after_bp"], out["messages_after_demod"], out["messages_after_ap"] = int(hb3[:, 0].sum()), int(n1.sum()), int(n2.sum())
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0 if out["records_equal_decode_messages_demod"] else 1


if __name__ == "__main__":
    sys.exit(main())
