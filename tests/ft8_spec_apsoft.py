"""CPU restatement of a-priori decoding on the soft bits demodulated from the I/Q samples (ft8gpu_demod_soft,
ft8gpu_ap_soft_candidates, ft8gpu_decode_messages_demod_ap; include/ft8gpu.h "a-priori decoding on the soft bits demodulated from
the I/Q samples", DESIGN.md "A-priori decoding on the demodulated soft bits").  Nothing here is new arithmetic: the rows are
tests/ft8_spec_demod.py's x, the per-row rule is tests/ft8_spec_ap.py's attempts / resolve, the append step is
tests/ft8_spec_multipass.py's.  The device compares byte for byte.

  soft [B][cap][3][176] float32, row n - 1 = set n: x (the output of ftx_normalize_logl the set's bp_decode ran on) where the
    candidate was attempted, the set is named, no earlier set was accepted and the set's result is not 6; 176 times +0 elsewhere
  AP: a qualifying candidate (ok == 0, ldpc_errors != 0) walks the named sets in ascending n; a row with a non-finite value or
    max |row| == 0 is unusable (code 6 in results[n - 1][0]); on a usable row the hypotheses run in table order by AP's rule with
    llr = the row as it stands; the first accepted (set, hypothesis) ends the candidate; no usable set: result 6, set 0"""
import numpy as np

import ft8_spec_ap as sa
import ft8_spec_demod as sdm
import ft8_spec_osd as so

F32 = np.float32
STRIDE = 176                                 # FT8GPU_SOFT_STRIDE
INFO_DTYPE = np.dtype([("result", "u1"), ("nhard", "u1"), ("hyp", "u1"), ("iters", "u1"), ("set", "u1"), ("pad", "u1", (3,)),
                       ("results", "u1", (3, 4))])
assert INFO_DTYPE.itemsize == 20 and INFO_DTYPE.fields["results"][1] == 8
MAX_HARD_ERRORS = 174                       # FT8GPU_APSOFT_MAX_HARD_ERRORS


def soft_rows(oracle, analysis, sets, gate=sdm.MAX_HARD_ERRORS):
    """the three rows of an attempted candidate from ft8_spec_demod.analyse()'s result -> float32 [3][176]"""
    rows = np.zeros((3, STRIDE), F32)
    _e, _d, _psync, per_set = analysis
    for n in (1, 2, 3):
        if not (sets >> (n - 1)) & 1:
            continue
        _llr, x, plain, errors = per_set[n]
        if x is None:                                              # result 6: a zero row
            continue
        rows[n - 1, :174] = x
        if sdm.judge(oracle, plain, errors, x, gate)[0] == 1:      # the accepted set's own row is written, later ones are not reached
            break
    return rows


def demod_soft(oracle, iq, cands, counts, status_in, sets=sdm.SETS, gate=sdm.MAX_HARD_ERRORS, max_per_frame=None, status_out=None,
               info=None, soft=None, iters=20, bp=None, w4=None, cache=None):
    """ft8gpu_demod_soft -> (status_out, info) of ft8_spec_demod.demod_candidates and soft float32 [B][cap][3][176]; rows at and
    behind counts[f] keep what `soft` held (zeros when None)"""
    import rtlsdr_ft8d_amd as ft8
    cache = {} if cache is None else cache
    out, inf = sdm.demod_candidates(oracle, iq, cands, counts, status_in, sets, gate, max_per_frame, status_out, info, iters, bp, w4, cache)
    B, cap = inf.shape
    rows = np.zeros((B, cap, 3, STRIDE), F32) if soft is None else np.array(soft, F32, copy=True).reshape(B, cap, 3, STRIDE)
    st = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, cap, 48).view(ft8.STATUS_DTYPE).reshape(B, cap)
    max_per_frame = cap if max_per_frame is None else max_per_frame
    for f in range(B):
        attempted = 0
        for i in range(int(counts[f])):
            rows[f, i] = 0
            if not (st[f, i]["ok"] == 0 and st[f, i]["ldpc_errors"] != 0) or attempted >= max_per_frame:
                continue
            attempted += 1
            rows[f, i] = soft_rows(oracle, cache[(f, cands[f, i].tobytes())], sets, gate)
    return out, inf, rows


def ap_soft_one(oracle, rows, sets, hyps, gate, iters=20, bp=None):
    """one qualifying candidate -> (info record, None or (plain, ext, calc, rc, text))"""
    info = np.zeros(1, INFO_DTYPE)[0]
    info["result"] = 6                                             # what stays when no set is usable
    for n in (1, 2, 3):
        if not (sets >> (n - 1)) & 1:
            continue
        row = np.asarray(rows[n - 1][:174], F32)
        tried = sa.attempts(oracle, row, hyps, iters, bp)
        if tried is None:
            info["results"][n - 1][0] = 6
            continue
        r, win = sa.resolve(oracle, row, tried, gate)
        info["result"], info["nhard"], info["hyp"], info["iters"], info["set"] = r["result"], r["nhard"], r["hyp"], r["iters"], n
        info["results"][n - 1] = r["results"]
        if win is not None:
            return info, win
    return info, None


def ap_soft_candidates(oracle, soft, counts, status_in, sets, hyps, gate, status_out=None, info=None, iters=20, bp=None):
    """ft8gpu_ap_soft_candidates: soft [B][cap][3][176], counts [B], status_in uint8 [B][cap][48] (or STATUS_DTYPE) ->
    (status_out uint8 [B][cap][48], info INFO_DTYPE [B][cap]).  Records at and behind counts[f] keep what status_out / info held
    (zeros when None)."""
    import rtlsdr_ft8d_amd as ft8
    assert sa.validate(hyps) and 1 <= sets <= 7
    B = len(counts)
    sin = np.ascontiguousarray(status_in).view(np.uint8).reshape(B, -1, 48)
    cap = sin.shape[1]
    soft = np.ascontiguousarray(soft, F32).reshape(B, cap, 3, STRIDE)
    out = np.zeros((B, cap, 48), np.uint8) if status_out is None else np.array(status_out, copy=True).view(np.uint8).reshape(B, cap, 48)
    inf = np.zeros((B, cap), INFO_DTYPE) if info is None else np.array(info, copy=True).view(INFO_DTYPE).reshape(B, cap)
    st = sin.view(ft8.STATUS_DTYPE).reshape(B, cap)
    for f in range(B):
        for i in range(int(counts[f])):
            out[f, i] = sin[f, i]
            inf[f, i] = np.zeros(1, INFO_DTYPE)[0]
            if st[f, i]["ok"] != 0 or st[f, i]["ldpc_errors"] == 0:
                continue
            inf[f, i], win = ap_soft_one(oracle, soft[f, i], sets, hyps, gate, iters, bp)
            if win is not None:
                plain, ext, calc, rc, text = win
                rec = np.zeros(1, ft8.STATUS_DTYPE)[0]
                rec["ldpc_errors"] = 0
                rec["iters"] = st[f, i]["iters"]
                rec["crc_extracted"], rec["crc_calculated"] = ext, calc
                rec["unpack_status"], rec["ok"] = rc, 1
                rec["a91"] = so.a91_of(plain)
                rec["text"] = text
                out[f, i] = np.frombuffer(rec.tobytes(), np.uint8)
    return out, inf


def decode_demod_ap(oracle, iq, sets=sdm.SETS, gate=sdm.MAX_HARD_ERRORS, max_per_frame=None, hyps=(), ap_gate=MAX_HARD_ERRORS, msgs=None,
                    max_candidates=120, min_score=10, nthreads=8, iters=20, stages=None, bp=None, trace=None, cache=None):
    """ft8gpu_decode_messages_demod_ap for iq [B][2][48000] -> (msgs [B][50], n [B], n_by_stage [B][3]): the records of
    ft8_spec_demod.decode_demod, AP on the rows of what is still undecoded, in place on the status records, and the append step on
    what it accepted (pad[1] = 1 + hypothesis, pad[3] = set).  hyps empty: no AP.  trace: receives (demod info, AP info or None)."""
    import ft8_spec_messages as sm
    import ft8_spec_multipass as mp
    iq = np.ascontiguousarray(iq, F32).reshape(-1, 2, sdm.NSAMPLES)
    B = iq.shape[0]
    cache = {} if cache is None else cache
    stages = stages if stages is not None else sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    dinfo = []
    o2, n2, nbs2 = sdm.decode_demod(oracle, iq, sets, gate, max_per_frame, msgs, max_candidates, min_score, nthreads, iters, stages, bp,
                                    dinfo, cache)
    nbs = np.zeros((B, 3), np.int32)
    nbs[:, :2] = nbs2
    nbs[:, 2] = n2
    ainfo = None
    if len(hyps):
        mag, cands, counts, status = stages
        st2, _inf, soft = demod_soft(oracle, iq, cands, counts, status, sets, gate, max_per_frame, iters=iters, bp=bp, cache=cache)
        st3, ainfo = ap_soft_candidates(oracle, soft, counts, st2, sets, hyps, ap_gate, iters=iters, bp=bp)
        o3, n3 = mp.append(mag, sm.noise_baseline(mag), cands, counts, st3, o2, n2, min_score=min_score)
        for f in range(B):
            for r in range(int(n2[f]), int(n3[f])):
                rec = ainfo[f, int(o3[f, r]["cand_index"])]
                o3[f, r]["pad"][1] = 1 + int(rec["hyp"])
                o3[f, r]["pad"][3] = rec["set"]
        o2, n2 = o3, n3
        nbs[:, 2] = n3
    if trace is not None:
        trace.append((dinfo[0], ainfo))
    return o2, n2, nbs
