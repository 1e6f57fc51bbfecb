"""Ground truth for ft8gpu_rx_stream: the oracle's ft8o_rx_callback driven the way the reference's daemon drives
rtlsdr_callback() -- the filter state carried from one slot into the next, a fresh iqIndex per slot -- followed by the
decoder thread's tail zeroing and optional peak normalisation, as in ft8o_rx_capture."""
import ctypes as C

import numpy as np

import oracle_lib

NS = 48000
# ft8o_rx_state_t (oracle/ft8_oracle.h), field for field
ORACLE_STATE_DTYPE = np.dtype([(n, "<i4") for n in ("Ix1", "Ix2", "Qx1", "Qx2", "Iy1", "It1y", "It1z", "Qy1", "Qt1y", "Qt1z",
                                                    "Iy2", "It2y", "It2z", "Qy2", "Qt2y", "Qt2z")]
                              + [("decimationIndex", "<u4"), ("firI", "<f4", (56,)), ("firQ", "<f4", (56,))])
FILL = 0xA5


def _lib():
    L = oracle_lib.lib()
    L.ft8o_rx_reset.argtypes = [C.c_void_p]
    L.ft8o_rx_reset.restype = None
    L.ft8o_rx_callback.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ft8o_rx_callback.restype = None
    L.ft8o_normalise.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.ft8o_normalise.restype = None
    return L


def reset_state():
    st = np.full(1, FILL, np.uint8).repeat(ORACLE_STATE_DTYPE.itemsize).view(ORACLE_STATE_DTYPE)
    _lib().ft8o_rx_reset(st.ctypes.data)
    return st


def oracle_slot(st, raw, normalise=False):
    """one slot: rtlsdr_callback over `raw` (uint8 [2*npairs]) from the state `st` (updated in place) with iqIndex = 0,
    then tail zeroing and normalisation.  -> (frame float32 [2][48000], stored count)"""
    L = _lib()
    buf = np.array(raw, np.uint8, copy=True)                  # the callback rewrites its buffer
    assert buf.ndim == 1 and buf.size % 16 == 0
    frame = np.full((2, NS), FILL, np.uint8).repeat(4, axis=1).view(np.float32)
    idx = C.c_uint32(0)
    L.ft8o_rx_callback(st.ctypes.data, buf.ctypes.data, buf.size, frame[0].ctypes.data, frame[1].ctypes.data, C.byref(idx))
    frame[:, idx.value:] = 0.0                                # rtlsdr_ft8d.c:243-246
    if normalise:
        L.ft8o_normalise(frame[0].ctypes.data, frame[1].ctypes.data, NS)
    return frame, idx.value


def oracle_chain(raw, state=None, normalise=False):
    """raw: uint8 [nslots][2*npairs], consecutive buffers of one receiver; state: ORACLE_STATE_DTYPE [1] or None (reset).
    -> (frames float32 [nslots][2][48000], counts uint32 [nslots], exit state [1]); `state` itself is not changed"""
    raw = np.ascontiguousarray(raw, np.uint8)
    st = reset_state() if state is None else np.array(state, ORACLE_STATE_DTYPE, copy=True).reshape(1)
    frames = np.empty((raw.shape[0], 2, NS), np.float32)
    counts = np.empty(raw.shape[0], np.uint32)
    for s in range(raw.shape[0]):
        frames[s], counts[s] = oracle_slot(st, raw[s], normalise)
    return frames, counts, st


def oracle_streams(raw, states=None, normalise=False):
    """raw: [nstreams][nslots][2*npairs]; states: [nstreams] or None -> (frames [nstreams][nslots][2][48000], counts, states)"""
    out = [oracle_chain(raw[k], None if states is None else states[k:k + 1], normalise) for k in range(raw.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.concatenate([o[2] for o in out])


def state_after(raw):
    """the oracle's state after a prefix `raw` (uint8 [2*npairs]) from reset"""
    st = reset_state()
    oracle_slot(st, raw)
    return st


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pattern(shape, dtype):
    """an output array pre-filled with 0xA5 bytes, so that an unwritten element shows"""
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = FILL
    return a
