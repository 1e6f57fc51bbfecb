"""CPU restatement of multi-pass decoding (ft8gpu_decode_messages_passes / ft8gpu_mask_messages / ft8gpu_append_messages,
DESIGN.md "Multi-pass decoding") in numpy, fed by the oracle's waterfall / find_sync / decode.  The mask follows the rule
literally -- pass p+1 masks W(p) with the records first written in pass p -- where the device masks the first pass's
waterfall with every record so far; the two agree because a masked cell always takes the baseline of its column.  Records
are built by tests/ft8_spec_messages.py's snr_parts / snr_db with the pass-1 baseline, so they compare byte for byte."""
import numpy as np

import ft8_spec_messages as sm

MAX_MESSAGES = sm.MAX_MESSAGES
MAG_ARRAY = sm.MAG_ARRAY


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def _status_view(status, B):
    import rtlsdr_ft8d_amd as ft8
    st = np.ascontiguousarray(status)
    if st.dtype != ft8.STATUS_DTYPE:
        st = st.view(np.uint8).reshape(B, -1, 48).view(ft8.STATUS_DTYPE).reshape(B, -1)
    return st


def mask(mag, base, msgs, first, n_msgs):
    """ft8gpu_mask_messages: mag [B][94208] with, for every symbol k of every record r in [first[f], n_msgs[f]) (clamped to
    [0, 50]) whose block to + k lies in [0, 92), the cell (to + k, ts, fs, fo + tone_k) set to base[f][fs][fo + tone_k];
    ts, fs = time_sub, freq_sub mod 2, fo = freq_offset clamped to [0, 248]"""
    out = np.array(np.asarray(mag, np.uint8).reshape(-1, MAG_ARRAY), copy=True)
    base = np.asarray(base, np.uint8).reshape(-1, 2, 256)
    for f in range(out.shape[0]):
        for r in range(_clamp(first[f], 0, MAX_MESSAGES), _clamp(n_msgs[f], 0, MAX_MESSAGES)):
            rec = msgs[f, r]
            c = rec["cand"]
            to, ts, fs = int(c["time_offset"]), int(c["time_sub"]) & 1, int(c["freq_sub"]) & 1
            fo = _clamp(c["freq_offset"], 0, 248)
            tones = sm.tones_of(rec["a91"])
            for k in range(79):
                if 0 <= to + k < 92:
                    b = fo + int(tones[k])
                    out[f, (to + k) * 1024 + ts * 512 + fs * 256 + b] = base[f, fs, b]
    return out


def _key(text_raw, h):
    return (int(h), sm._c_text(text_raw))


def append(mag, base, cands, counts, status, msgs, n_msgs, min_score=10):
    """ft8gpu_append_messages: the pass's unique messages in candidate order, those not yet among the frame's records
    [0, n_msgs[f]) (clamped to [0, 50]) appended behind them up to 50; snr_db from this pass's waterfall `mag` and the
    pass-1 baseline `base`.  Returns new (msgs, n)."""
    import rtlsdr_ft8d_amd as ft8
    mag = np.ascontiguousarray(mag, np.uint8).reshape(-1, MAG_ARRAY)
    B = mag.shape[0]
    base = np.asarray(base, np.uint8).reshape(-1, 2, 256)
    st = _status_view(status, B)
    raw = st.view(np.uint8).reshape(B, -1, 48)
    out = np.array(msgs, copy=True)
    n = np.zeros(B, np.int32)
    for f in range(B):
        n0 = _clamp(n_msgs[f], 0, MAX_MESSAGES)
        seen = [_key(out[f, r].tobytes()[:25], out[f, r]["hash"]) for r in range(n0)]
        kept = n0
        for i in range(_clamp(counts[f], 0, st.shape[1])):            # idx < max_candidates && idx < counts[f]
            if kept >= MAX_MESSAGES:
                break
            c, r = cands[f, i], st[f, i]
            if int(c["score"]) < min_score or r["ok"] == 0:
                continue
            text_raw = raw[f, i, 22:47].tobytes()
            key = _key(text_raw, r["crc_extracted"])
            if key in seen:
                continue
            seen.append(key)
            a91 = raw[f, i, 10:22].tobytes()
            S, nsym, nb = sm.snr_parts(mag[f], base[f], c, sm.tones_of(a91))
            rec = np.zeros(1, ft8.MESSAGE_DTYPE)[0]
            rec["text"] = text_raw
            rec["snr_db"] = sm.snr_db(S, nsym, nb)
            rec["score"] = c["score"]
            rec["freq_hz"] = (np.float32(c["freq_offset"]) + np.float32(c["freq_sub"]) / np.float32(2)) * np.float32(6.25)
            rec["dt_s"] = (np.float32(c["time_offset"]) + np.float32(c["time_sub"]) / np.float32(2)) / np.float32(6.25)
            rec["hash"] = r["crc_extracted"]
            rec["cand_index"] = i
            rec["cand"] = c
            rec["a91"] = np.frombuffer(a91, np.uint8)
            out[f, kept] = rec
            kept += 1
        n[f] = kept
    return out, n


def decode_passes(oracle, iq, passes, max_candidates=120, min_score=10, nthreads=8, msgs=None, stages=None, iters=20):
    """the whole path for B frames [B][2][48000] -> (msgs [B][50], n [B], n_by_pass [B][passes]).
    stages: the first pass's oracle stages (mag, cands, counts, status) when the caller has them already."""
    import rtlsdr_ft8d_amd as ft8
    mag, cands, counts, status = stages if stages is not None else sm.oracle_stages(oracle, iq, max_candidates, min_score, nthreads, iters)
    B = mag.shape[0]
    out, n = sm.collect(mag, cands, counts, status, min_score=min_score,
                        msgs=np.zeros((B, MAX_MESSAGES), ft8.MESSAGE_DTYPE) if msgs is None else msgs)
    base = sm.noise_baseline(mag)
    nbp = np.zeros((B, passes), np.int32)
    nbp[:, 0] = n
    W = np.array(mag, copy=True)
    prev = np.zeros(B, np.int32)                       # counts before the last pass
    for p in range(1, passes):
        active = [f for f in range(B) if prev[f] < n[f] < MAX_MESSAGES]
        if active:
            a = np.array(active)
            W[a] = mask(W[a], base[a], out[a], prev[a], n[a])
            c2, k2 = oracle.find_sync_batch(W[a], max_candidates, min_score, nthreads=nthreads)
            s2 = oracle.decode_candidates_batch(W[a], c2, k2, iters=iters, nthreads=nthreads)
            prev = n.copy()
            o2, n2 = append(W[a], base[a], c2, k2, s2, out[a], n[a], min_score=min_score)
            out[a], n[a] = o2, n2
        else:
            prev = n.copy()
        nbp[:, p] = n
    return out, n, nbp


def planted_hits(msgs, n, planted):
    """(decodes whose text is among the frame's planted messages, decodes that are not) over a batch"""
    hit = miss = 0
    for f in range(len(n)):
        want = set(t for t in planted[f] if t is not None)
        for r in msgs[f, :int(n[f])]:
            if r["text"].decode(errors="replace") in want:
                hit += 1
            else:
                miss += 1
    return hit, miss
