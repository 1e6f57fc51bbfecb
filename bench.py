#!/usr/bin/env python3
"""bench.py -- frames decoded per second by the MI355X FT8 hot path (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W                       (configs[2], the default)
  python bench.py --config 4                                          (configs[4]: oversubscribed candidate set)
  python bench.py --config 1                                          (configs[1]: GPU waterfall + sync, LDPC on the CPU)
  python bench.py --gpus N --steps K --warmup W                       (N > 1 without RANK/WORLD_SIZE in the environment:
                                                                       bench.py starts its own N ranks, see self_launch)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W
  python bench.py --config 3                                          (configs[3]: 8 shards of 4096 frames; --gpus 8 = one shard per
                                                                       GPU + RCCL gather, --gpus 1 = the 8 shards as 8 contexts on one GPU)
  python bench.py --gpus 2 --backend gloo --dry                       (launcher / sharding / exchange check without a GPU)
  python bench.py --gpus 1 --steps K --warmup W --full                (+ per-kernel roofline, shader clock, CPU baseline,
                                                                       PCIe-inclusive host legs and the workload checks)
  python bench.py ... --dump-outputs DIR                              (the last timed step's records as DIR/*.npy)

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step, ...); everything else it can measure or check runs only with --full.

A step = one pass of the whole decode path (waterfall FFT -> Costas sync -> LLR -> LDPC BP -> CRC ->
unpack -> dedup/spots) over the rank's batch of synthetic 15 s frames, resident in HBM before the
timed region starts.  Frames are independent, so N GPUs each take a contiguous shard of the global
batch (weak scaling: frames per GPU fixed); the only collective is one RCCL all-gather of the
fixed-size spot records per step, double-buffered so that it runs under the next step's kernels.
Prints ONE JSON line on rank 0.

configs[1] is the split BASELINE.json describes -- waterfall and sync search on the GPU, their results
(94 208 B waterfall + 964 B candidate list per frame) copied to the host, LLR / BP / CRC / unpack / dedup on
the host cores.  The host half has no product implementation (the product decodes on the GPU): it is the
CPU oracle, i.e. this mode measures "GPU front end + reference-style CPU back end", and says so in its line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BYTES_PER_FRAME = 384000 + 1404          # IQ in + 50 spot records and the count out
BYTES_PER_FRAME_CFG1 = 384000 + 94208 + 964   # configs[1]: IQ in + waterfall and candidate list out
HBM_PEAK_GBPS = 8000.0                   # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_COPY_PEAK_GBPS = 6290.0              # same guide: measured copy peak (SURVEY.md 8(d) asks for both)
FP32_VALU_PEAK = 157.3e12                # same guide: fp32 vector peak, flop/s (an FMA lane-instruction counts 2)

CONFIGS = {
    1: dict(frames=256, nsig=20, snr=(-18.0, 0.0), max_candidates=120,
            label="configs[1]: batch of {B} synthetic frames, {S} CQ signals/frame SNR U[{lo:g},{hi:g}] dB, waterfall + sync "
                  "(+ exact top-{C} heap) on the GPU, D2H of waterfall + candidates, LDPC/CRC/unpack/dedup on the host cores (CPU oracle)"),
    2: dict(frames=4096, nsig=20, snr=(-18.0, 0.0), max_candidates=120,
            label="configs[2]: batch of {B} synthetic 15 s 3200 sps IQ frames per GPU, {S} CQ signals/frame SNR U[{lo:g},{hi:g}] dB, "
                  "full pipeline incl. HIP LDPC(174,91) BP, K_MAX_CANDIDATES={C}"),
    3: dict(frames=4096, nsig=20, snr=(-18.0, 0.0), max_candidates=120,
            label="configs[3]: 32768 synthetic frames as 8 contiguous shards of {B}, {S} CQ signals/frame SNR U[{lo:g},{hi:g}] dB, full pipeline, "
                  "K_MAX_CANDIDATES={C}, spot records gathered"),
    4: dict(frames=1024, nsig=60, snr=(-24.0, -14.0), max_candidates=480,
            label="configs[4]: oversubscribed candidate set, batch of {B} synthetic frames per GPU, {S} weak CQ signals/frame "
                  "SNR U[{lo:g},{hi:g}] dB, K_MAX_CANDIDATES x4 = {C}, full pipeline incl. HIP LDPC(174,91) BP"),
}

DUMP_MAX_FRAMES = 8192                   # --dump-outputs writes 6 416 B per frame: 52.6 MB at most


def dump_outputs(path, records, counts):
    """--dump-outputs: what a caller of the timed path received from its last step, as .npy files in `path`:
      records.npy      [frames, 50, 28] float32  every byte of the caller's record array (RESULT_DTYPE slots: call, loc, freq, snr;
                                                 slots past the count hold what the array held before, zeros here)
      freq.npy, snr.npy  [frames, 50] float64    the two integer fields of every slot
      n_results.npy    [frames] float64          messages per frame
      frame_index.npy  [frames] float64          the frame each row is (rows are all frames, or a sorted sample of them)
    Beyond DUMP_MAX_FRAMES frames a fixed, seeded sample of the frames is written, the same on every run."""
    import rtlsdr_ft8d_amd as ft8
    counts = np.asarray(counts)
    rec = np.ascontiguousarray(records).view(np.uint8).reshape(len(counts), ft8.MAX_MESSAGES, ft8.RESULT_DTYPE.itemsize)
    idx = np.arange(len(counts))
    if len(idx) > DUMP_MAX_FRAMES:
        idx = np.sort(np.random.default_rng(0).choice(len(idx), DUMP_MAX_FRAMES, replace=False))
    rec = np.ascontiguousarray(rec[idx])
    slots = rec.view(ft8.RESULT_DTYPE).reshape(len(idx), ft8.MAX_MESSAGES)
    arrays = {"records": rec.astype(np.float32), "freq": slots["freq"].astype(np.float64), "snr": slots["snr"].astype(np.float64),
              "n_results": counts[idx].astype(np.float64), "frame_index": idx.astype(np.float64)}
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {"dir": path, "frames": int(len(idx)), "of_frames": int(len(counts)), "bytes": int(sum(a.nbytes for a in arrays.values())),
            "files": sorted(name + ".npy" for name in arrays)}


def csrc_hash():
    """identity of the kernel sources the committed PMC summaries were collected on: the device half of the library's
    build id (csrc/*.hip, *.h; host-only .c files do not change a kernel)"""
    import rtlsdr_ft8d_amd as ft8
    return ft8.device_source_id()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", type=int, choices=(1, 2, 3, 4), default=2, help="index into BASELINE.json configs (default 2: the metric's configuration)")
    ap.add_argument("--frames", type=int, default=None, help="frames per GPU per step (default: the config's)")
    ap.add_argument("--nsig", type=int, default=None, help="FT8 signals per frame")
    ap.add_argument("--snr", type=float, nargs=2, default=None)
    ap.add_argument("--max-candidates", type=int, default=None)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the per-kernel stage timings and roofline, the shader clock / power sampler, the workload "
                         "checks (messages and CQ spots per frame), the CPU baseline and the PCIe-inclusive host legs; a plain run does none of it")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last one computed (spot records and counts) as float32 / float64 .npy files to "
                         "DIR (a fixed, seeded sample of frames beyond %d frames: at most 64 MB in all)" % DUMP_MAX_FRAMES)
    ap.add_argument("--cpu-frames", type=int, default=2048, help="--full: frames timed on the host CPU (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-host-legs", action="store_true", help="--full: skip the PCIe-inclusive end-to-end legs (host-fed decode, raw-capture replay)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise RCCL and run the spot all-gather even with one rank (exercises the N>1 code path on one GPU)")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="process-group backend (nccl = RCCL; gloo only with --dry)")
    ap.add_argument("--dry", action="store_true",
                    help="no GPU work: every rank fills its shard's spot buffers with a pattern derived from the global frame index and "
                         "runs the real exchange; checks launcher, sharding and gather (CPU tensors, gloo)")
    ap.add_argument("--prewarm", type=int, default=8,
                    help="untimed steps run before the W warm-up steps: after any idle period the GPU needs about 30 ms of load to "
                         "reach its sustained clock (per-step times from cold: 5.65, 4.82, 4.67, 4.54, 4.48, 4.38, 4.25, 4.25 ... ms, "
                         "tools/perstep_probe.py), which short --warmup values would put inside the timed region; reported in the line")
    ap.add_argument("--prewarm-seconds", type=float, default=1.0,
                    help="after the --prewarm steps keep running untimed steps for about this long before the W warm-up steps (the step count is "
                         "fixed from a short calibration, the same on every rank): on some boxes of the pool the shader clock is still settling "
                         "0.1 s after idle -- a 60 s run of the same loop was 2.2 %% faster than the 80 ms timed region that preceded it on one box, "
                         "equal on another (profiles/r06_bench_sustained_60s*.json) -- so the timed region starts from the state a replay job "
                         "runs in; the steps actually run are reported as prewarm_steps")
    ap.add_argument("--no-clock-sampler", action="store_true",
                    help="do not poll the GPU's sysfs clock / power files (during the timed region with --full, during --sustain-seconds)")
    ap.add_argument("--ctx-last", action="store_true",
                    help="create the decoder context AFTER the process group and a handful of framework streams (round 3 lost 0.27 ms per step "
                         "that way: streams shared hardware queues; the context now measures co-execution and re-rolls its side streams)")
    ap.add_argument("--debug-flags", type=int, default=0,
                    help="FT8GPU_DBG_* bits for the decoder context (reported in the line, 0 = product); the kernel-form selectors 8 / 16 / 32 "
                         "need --ab-lib")
    ap.add_argument("--ab-lib", action="store_true",
                    help="run on the A/B build libft8gpu_ab.so (product kernels + the alternative kernel forms; `make -C rtlsdr_ft8d_amd/csrc ab`): "
                         "profiling of the non-product forms only, reported in the line")
    ap.add_argument("--shards", type=int, default=8, help="configs[3] on one GPU: number of contexts / shards")
    ap.add_argument("--sustain-seconds", type=float, default=0.0,
                    help="after the timed K steps (the headline, unchanged) keep running the same step loop for about this many seconds and add a "
                         "`sustained` object to the line: rate, per-step p50 / p99, first-second against last-second rate, shader clock, socket power and "
                         "temperatures over time (the headline is an 80 ms window on a power-limited kernel; this is the operating regime of a replay job)")
    ap.add_argument("--dist-timeout", type=float, default=180.0,
                    help="multi-rank runs: seconds any one phase (process-group init, first collective, ...) may take before the rank's watchdog "
                         "process reports the rank and phase in a JSON line and kills the rank; also the process group's own timeout")
    ap.add_argument("--no-exchange", action="store_true",
                    help="multi-rank control leg: the ranks decode their shards with NO collective in the step (barrier and timing reduction only), so "
                         "that a scaling curve separates decode scaling from the cost of the spot gather")
    ap.add_argument("--test-hang", default=None, metavar="RANK:PHASE[:SECONDS]",
                    help="test hook: that rank sleeps forever when it enters that phase (what a hung RCCL init looks like to the watchdog); "
                         "SECONDS = the watchdog limit of that phase only")
    ap.add_argument("--test-fail-exchange", default=None, metavar="RANK:STEP",
                    help="test hook: that rank's exchange raises at that step (what a failing collective looks like to the error path)")
    ap.add_argument("--traffic", choices=("cq", "mixed"), default="cq",
                    help="message pool of the synthetic frames: cq = 'CQ call grid' only (SURVEY.md 8(d), the headline); mixed = what a receiver "
                         "meets on the air (workload.mixed_message_pool: about a quarter CQ calls, the rest QSO traffic of every message type, one "
                         "frame in four with a message heard twice) -- a side line, reported as such")
    return ap.parse_args(argv)


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no RANK/WORLD_SIZE in the environment: start the N ranks as fresh
    child processes through torch.distributed.run (one per GPU, rendezvous on 127.0.0.1 and a free port), BEFORE this
    process has imported torch or made any GPU call, relay rank 0's single JSON line and exit with the children's
    status.  The children see RANK/LOCAL_RANK/WORLD_SIZE and run main() as the driver's own torchrun command would."""
    import subprocess
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    env["FT8_BENCH_SELF_LAUNCHED"] = "1"
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith('{"metric"'):
            line = ln
    if p.returncode != 0 or line is None:
        sys.stderr.write(p.stderr[-6000:])
        sys.stderr.write(p.stdout[-2000:])
        sys.stderr.write(f"\nbench.py: the {args.gpus}-rank job failed (exit {p.returncode}, JSON line {'found' if line else 'missing'})\n")
        for ln in p.stdout.splitlines():            # the diagnosis a failing or hanging rank (or its watchdog) left: relay every such line
            if ln.startswith('{"metric"') and '"failed": true' in ln:
                emit(ln)
        raise SystemExit(p.returncode or 1)
    emit(line)
    raise SystemExit(0)


METRIC = "15 s FT8 frames decoded/s"

# One small child process per rank (started before the rank imports torch or touches the GPU; never an exec of the rank itself).
# The rank tells it "phase <name> <seconds>" on a pipe; when a phase outlives its limit -- a hung RCCL init holds no Python
# thread the rank could rely on -- the child prints ONE JSON line naming rank and phase on the job's stdout, says the same on
# stderr, and kills the rank, so that the launcher tears the job down with a non-zero status instead of waiting for ever.
WATCHDOG_CODE = r"""
import json, os, select, signal, sys, time
rank, world, ppid, metric = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
phase, deadline, since, buf, history, result = "start", None, time.time(), b"", [], None
while True:
    r, _, _ = select.select([0], [], [], None if deadline is None else max(0.0, deadline - time.time()))
    if r:
        chunk = os.read(0, 4096)
        if not chunk:
            sys.exit(0)                              # the rank is gone: it finished, or died on its own and said why itself
        buf += chunk
        while b"\n" in buf:
            ln, buf = buf.split(b"\n", 1)
            w = ln.decode().split(" ", 1)
            if w[0] == "done":
                sys.exit(0)
            if w[0] == "result":                     # the rank's measured line so far: printed in its place should it hang afterwards
                result = w[1]
                continue
            w = ln.decode().split(" ")
            history.append([phase, round(time.time() - since, 2)])
            phase, since = w[1], time.time()
            deadline = since + float(w[2])
    elif deadline is not None and time.time() >= deadline:
        waited = round(time.time() - since, 1)
        msg = {"metric": metric, "value": None, "unit": "frames/s", "n_gpus": world, "failed": True, "rank": rank, "phase": phase,
               "error": "rank %d of %d hung in phase '%s' for %.0f s (limit %.0f s); killed by its watchdog" % (rank, world, phase, waited, deadline - since),
               "phases_completed": history[1:], "pid": ppid}
        note = msg["error"]
        if result is not None:
            # the timed region was over and reduced when the rank hung: the measurement stands; say what did not complete
            line = json.loads(result)
            line.update({"completed": False, "hung_after_timing_in_phase": phase, "watchdog": note})
            msg = line
        sys.stdout.write(json.dumps(msg) + "\n"); sys.stdout.flush()
        sys.stderr.write("bench.py watchdog: " + note + "\n"); sys.stderr.flush()
        try:
            os.kill(ppid, signal.SIGKILL)
        except OSError:
            pass
        sys.exit(3)
"""


class RankWatchdog:
    def __init__(self, rank, world, enabled, default_timeout):
        self.rank, self.default_timeout, self.p, self.current = rank, default_timeout, None, "start"
        if enabled:
            import subprocess
            self.p = subprocess.Popen([sys.executable, "-c", WATCHDOG_CODE, str(rank), str(world), str(os.getpid()), METRIC], stdin=subprocess.PIPE)

    def phase(self, name, timeout=None):
        self.current = name
        if self.p:
            try:
                self.p.stdin.write(f"phase {name} {timeout or self.default_timeout}\n".encode())
                self.p.stdin.flush()
            except OSError:
                pass

    def result(self, line):
        """deposit the rank's measured line: should the rank hang in a later phase, the watchdog prints it (marked incomplete)"""
        if self.p:
            try:
                self.p.stdin.write(b"result " + json.dumps(line).encode() + b"\n")
                self.p.stdin.flush()
            except OSError:
                pass

    def done(self):
        if self.p:
            try:
                self.p.stdin.write(b"done\n")
                self.p.stdin.flush()
                self.p.stdin.close()
            except OSError:
                pass
            self.p.wait(timeout=10)
            self.p = None


def _rank_step(spec):
    """'R:X' test-hook argument -> (R, 'X') or None"""
    if not spec:
        return None
    r, x = spec.split(":", 1)
    return int(r), x


def _hang_spec(spec):
    """--test-hang 'RANK:PHASE[:SECONDS]' -> ((RANK, PHASE), seconds or None): the optional third field is the watchdog limit of
    THAT phase only, so that a test can keep a generous --dist-timeout for the real phases (a cold RCCL load takes a while)"""
    if not spec:
        return None, None
    f = spec.split(":")
    return (int(f[0]), f[1]), (float(f[2]) if len(f) > 2 else None)


def store_publish(store, key, value):
    try:
        store.set(key, json.dumps(value))
    except Exception:                                        # diagnostics must never be what fails
        pass


def store_collect(store, prefix, world, wait_s=0.0):
    """what the ranks published under prefix<rank> (c10d store: TCP, no RCCL involved); ranks that did not are absent"""
    import datetime
    res = {}
    for r in range(world):
        try:
            if wait_s > 0:
                store.wait([f"{prefix}{r}"], datetime.timedelta(seconds=wait_s))
            elif not store.check([f"{prefix}{r}"]):
                continue
            res[str(r)] = json.loads(store.get(f"{prefix}{r}").decode())
        except Exception:
            continue
    return res


def emit(line):
    """print ONE JSON line as ONE write on stdout.  The ranks of a job share the pipe, and under torch.distributed.run their
    stdout is unbuffered: there print() writes the text and its newline separately, and another rank's line can land in
    between (two objects on one line, the newline later)."""
    sys.stdout.flush()
    data = (line + "\n").encode()
    while data:
        data = data[os.write(sys.stdout.fileno(), data):]


def failure_line(out, rank, world, phase, exc, store, extra=None):
    """the ONE line a rank prints when it fails after start-up: what failed, where, and what is known of every rank's decode rate"""
    txt = f"{type(exc).__name__}: {exc}"
    is_coll = type(exc).__name__ in ("DistBackendError", "DistNetworkError", "DistStoreError", "DistError") or any(w in txt for w in ("NCCL", "RCCL", "nccl", "rccl", "collective"))
    line = {"metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": world, "failed": True, "rank": rank, "phase": phase,
            ("rccl_error" if is_coll else "error"): txt[:2000], "config": out.get("config"), "build_id": out.get("build_id"), "backend": out.get("backend")}
    if store is not None:
        line["per_rank_decode_only"] = store_collect(store, "ft8/decode_only/", world)
        line["ranks_info"] = store_collect(store, "ft8/info/", world)
    line.update(extra or {})
    return json.dumps(line)


class ClockSampler:
    """best-effort shader clock / socket power (and, with temps=True, the hwmon temperatures) of GPU `index` while a region runs
    (sysfs, `period` seconds); every field is null when the box does not expose the files to an ordinary user"""

    def __init__(self, index, enabled=True, period=0.02, temps=False):
        import glob
        self.sclk, self.power, self.t = [], [], []
        self.temp = {}                                   # label -> [deg C], sampled with the clock
        self.clk_file = self.pow_file = None
        self.temp_files = {}
        self.period = period
        try:
            if not enabled:
                raise OSError("disabled")                                    # the box exposes every GPU of the host in sysfs: find ours by PCI address
            import torch
            pr = torch.cuda.get_device_properties(index)
            bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            d = os.path.join("/sys/bus/pci/devices", bdf)
            if os.path.exists(os.path.join(d, "pp_dpm_sclk")):
                self.clk_file = os.path.join(d, "pp_dpm_sclk")
                hw = sorted(glob.glob(os.path.join(d, "hwmon/hwmon*/power1_average"))) or \
                    sorted(glob.glob(os.path.join(d, "hwmon/hwmon*/power1_input")))
                self.pow_file = hw[0] if hw else None
                self.bdf = bdf
                if temps:
                    for f in sorted(glob.glob(os.path.join(d, "hwmon/hwmon*/temp*_input"))):
                        try:
                            with open(f.replace("_input", "_label")) as lf:
                                label = lf.read().strip()
                        except OSError:
                            label = os.path.basename(f).replace("_input", "")
                        self.temp_files[label] = f
                        self.temp[label] = []
        except (AttributeError, RuntimeError, OSError):
            pass
        self._stop = False
        self._t = None

    def _run(self):
        while not self._stop:
            try:
                now = time.perf_counter()
                with open(self.clk_file) as f:
                    for ln in f:
                        if "*" in ln:
                            self.sclk.append(float(ln.split(":")[1].lower().replace("mhz", "").replace("*", "").strip()))
                            self.t.append(now)
                if self.pow_file:
                    with open(self.pow_file) as f:
                        self.power.append(float(f.read()) * 1e-6)
                for label, path in self.temp_files.items():
                    try:
                        with open(path) as f:
                            self.temp[label].append(float(f.read()) * 1e-3)
                    except (OSError, ValueError):
                        self.temp[label].append(float("nan"))
            except (OSError, ValueError, IndexError):
                return
            time.sleep(self.period)

    def clear(self):
        for v in (self.sclk, self.power, self.t, *self.temp.values()):
            v.clear()

    def __enter__(self):
        if self.clk_file:
            import threading
            self._t = threading.Thread(target=self._run, daemon=True)
            self._t.start()
        return self

    def __exit__(self, *a):
        self._stop = True
        if self._t:
            self._t.join(timeout=1.0)

    def summary(self):
        med = lambda v: round(float(np.median(v)), 1) if v else None
        return {"sclk_mhz_median": med(self.sclk), "sclk_mhz_min": round(min(self.sclk), 1) if self.sclk else None,
                "power_w_median": med(self.power), "samples": len(self.sclk),
                "source": f"sysfs pp_dpm_sclk / hwmon power of {getattr(self, 'bdf', None)}, {self.period * 1e3:.0f} ms period over the timed region" if self.sclk else None}

    def series(self, t0, nbuckets, bucket_s=1.0):
        """per-bucket medians since t0: [{"sclk_mhz", "power_w", "temp_c": {label: v}}] (None where no sample fell)"""
        t = np.asarray(self.t) - t0
        k = np.floor(t / bucket_s).astype(int) if len(t) else np.zeros(0, int)
        rows = []
        for b in range(nbuckets):
            m = k == b
            pick = lambda v: round(float(np.nanmedian(np.asarray(v)[:len(m)][m[:len(v)]])), 1) if len(v) and m[:len(v)].any() else None
            rows.append({"sclk_mhz": pick(self.sclk), "power_w": pick(self.power), "temp_c": {lb: pick(v) for lb, v in self.temp.items()}})
        return rows


def dry_records(lo, hi, step):
    """the pattern a dry run exchanges: record bytes and count of global frame g at `step` depend on (g, step) only"""
    g = np.arange(lo, hi, dtype=np.int64)
    rec = ((g[:, None] * 131 + np.arange(1400)[None, :] * 7 + step) & 0xFF).astype(np.uint8)
    cnt = ((g * 3 + step) % 51).astype(np.int32)
    return rec, cnt


def run_dry(args, out, rank, world, B, total, lo, hi, store=None):
    """--dry: launcher + shard_range + SpotExchange on CPU tensors (gloo).  No decode, no GPU: `value` is not a
    decode rate and the line says so."""
    import torch
    import torch.distributed as dist
    from rtlsdr_ft8d_amd import workload
    exchange = world > 1 and not args.no_exchange
    exch = workload.SpotExchange(B, world, torch.device("cpu"), collective=exchange)
    steps = args.warmup + args.steps
    fail = _rank_step(args.test_fail_exchange)
    ok = True
    # what the GPU path publishes as a rank's decode-only rate before its first collective (here: the pattern fill)
    t = time.perf_counter()
    for k in range(3):
        dry_records(lo, hi, k)
    if store is not None:
        store_publish(store, f"ft8/decode_only/{rank}", {"frames_per_s": round(3 * B / max(time.perf_counter() - t, 1e-9), 1), "what": "dry-run pattern fill"})
    t0 = time.perf_counter()
    for k in range(steps):
        s_buf, n_buf = exch.buffers(k)
        rec, cnt = dry_records(lo, hi, k)
        s_buf.copy_(torch.from_numpy(rec))
        n_buf.copy_(torch.from_numpy(cnt))
        if fail and fail == (rank, str(k)):
            raise RuntimeError(f"simulated collective failure at step {k} (--test-fail-exchange)")
        exch.launch(k)
        if k >= 1:                                   # check the previous step's gather while this one is in flight
            gs, gc = exch.gathered(k - 1)
            er, ec = dry_records(0, total, k - 1) if exchange else dry_records(lo, hi, k - 1)
            ok = ok and bool((gs.numpy() == er).all()) and bool((gc.numpy() == ec).all())
    gs, gc = exch.gathered(steps - 1)
    er, ec = dry_records(0, total, steps - 1) if exchange else dry_records(lo, hi, steps - 1)
    ok = ok and bool((gs.numpy() == er).all()) and bool((gc.numpy() == ec).all())
    exch.wait_all()
    if world > 1:
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        ok = bool(flag.item())
        dist.barrier()
    elapsed = time.perf_counter() - t0
    out["value"] = round(total * steps / elapsed, 1)
    out["ms_per_step"] = round(1e3 * elapsed / steps, 3)
    out["data"] = "dry-run: no decode, pattern records through the real launcher / sharding / exchange"
    out["dry"] = True
    out["exchange"] = "all_gather_into_tensor per step" if exchange else "none"
    out["dry_gather_identical_on_all_ranks"] = ok
    return ok


def rank_info(torch, local_rank, gpu):
    """what first contact needs to know about a rank: which physical GPU it holds and what the process sees"""
    import socket
    info = {"pid": os.getpid(), "host": socket.gethostname(), "local_rank": local_rank,
            "env": {k: os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "HSA_ENABLE_IPC_MODE_LEGACY") if os.environ.get(k) is not None}}
    if gpu:
        try:
            pr = torch.cuda.get_device_properties(local_rank)
            info.update({"visible_devices": torch.cuda.device_count(), "device": pr.name,
                         "pci": f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"})
        except (AttributeError, RuntimeError):
            pass
        try:
            info["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            info["rccl_version"] = None
    return info


def run_sustained(args, torch, dist, step, fence, stream, local_rank, n_steps, B, world, use_dist, dev, headline_ms):
    """--sustain-seconds: the SAME step loop as the timed region, for n_steps (the same number on every rank: the exchange
    is a collective), without ever letting the GPU run dry: steps are enqueued a chunk ahead while the previous chunk's
    hipEvents are read.  Returns the `sustained` object (rank 0's GPU; frames_per_s is the whole job)."""
    CH = 64
    ring = [torch.cuda.Event(enable_timing=True) for _ in range(3 * CH)]
    start_ev = torch.cuda.Event(enable_timing=True)
    done_ms = np.zeros(n_steps)                       # completion time of every step since the start event

    def read(c0, c1):
        ring[(c1 - 1) % len(ring)].synchronize()
        for i in range(c0, c1):
            done_ms[i] = start_ev.elapsed_time(ring[i % len(ring)])

    with ClockSampler(local_rank, not args.no_clock_sampler, period=0.1, temps=True) as clk:
        fence()
        clk.clear()
        t0 = time.perf_counter()
        start_ev.record(stream)
        for c0 in range(0, n_steps, CH):
            c1 = min(c0 + CH, n_steps)
            for i in range(c0, c1):
                step()
                ring[i % len(ring)].record(stream)
            if c0 > 0:
                read(c0 - CH, c0)                     # the chunk before this one, while this one runs
        read((n_steps - 1) // CH * CH, n_steps)
        fence()
        wall = time.perf_counter() - t0
    tmax = torch.tensor([wall], dtype=torch.float64, device=dev)
    if use_dist:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    wall_all = float(tmax.item())
    per_step = np.diff(np.concatenate([[0.0], done_ms]))
    nsec = max(1, int(np.ceil(done_ms[-1] / 1e3)))
    sec = np.minimum((done_ms / 1e3).astype(int), nsec - 1)
    full = int(done_ms[-1] // 1e3)                    # complete seconds
    counts = np.bincount(sec, minlength=nsec)
    rate = [int(c) * B * world for c in counts]        # frames/s of the whole job by rank 0's clock (ranks run the same steps)
    trace = clk.series(t0, nsec)
    pct = lambda q: round(float(np.percentile(per_step, q)), 4)
    first, last = (rate[0], rate[full - 1]) if full >= 2 else (None, None)
    col = lambda key: [r[key] for r in trace if r[key] is not None]
    sclk, power = col("sclk_mhz"), col("power_w")
    temps = {lb: [r["temp_c"][lb] for r in trace if r["temp_c"].get(lb) is not None] for lb in (trace[0]["temp_c"] if trace else {})}
    stride = max(1, nsec // 60)
    # the first three seconds in 100 ms buckets: how long the clock takes to settle after whatever preceded the run
    early = []
    for b in range(30):
        m = (done_ms >= 100.0 * b) & (done_ms < 100.0 * (b + 1))
        if m.any():
            early.append(round(float(per_step[m].mean()), 4))
    return {
        "seconds": round(wall_all, 2), "steps": n_steps, "frames_per_s": round(B * world * n_steps / wall_all, 1),
        "ms_per_step": {"mean": round(1e3 * wall_all / n_steps, 4), "p50": pct(50), "p99": pct(99), "max": round(float(per_step.max()), 4), "min": round(float(per_step.min()), 4)},
        "headline_ms_per_step": round(headline_ms, 4), "sustained_vs_headline": round(headline_ms / (1e3 * wall_all / n_steps), 4),
        "first_second_frames_per_s": first, "last_second_frames_per_s": last,
        "last_vs_first_second": round(last / first, 4) if first else None,
        "sclk_mhz": {"min": min(sclk), "median": round(float(np.median(sclk)), 1), "first_second": sclk[0], "last_second": sclk[-1]} if sclk else None,
        "power_w": {"median": round(float(np.median(power)), 1), "max": max(power), "first_second": power[0], "last_second": power[-1]} if power else None,
        "frames_per_joule": round(B * n_steps / wall_all / float(np.median(power)), 1) if power else None,     # rank 0's GPU: its frames / its socket energy
        "temperature_c": {lb: {"first_second": v[0], "last_second": v[-1], "max": max(v)} for lb, v in temps.items() if v} or None,
        "first_3s_mean_ms_per_step_by_100ms": early,
        "per_second": [{"t": k, "frames_per_s": rate[k], **trace[k]} for k in range(0, full, stride)],
        "note": "same step loop as the timed region, run back to back (hipEvent per step, read a chunk behind so the queue never drains); per-second rows: "
                "steps completed in that second x frames, medians of the 100 ms sysfs samples of rank 0's GPU",
    }


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        self_launch(args)                       # does not return; nothing above has touched torch or the GPU
    cfg = CONFIGS[args.config]
    B = args.frames or cfg["frames"]
    nsig = cfg["nsig"] if args.nsig is None else args.nsig
    snr = tuple(args.snr) if args.snr else cfg["snr"]
    maxc = args.max_candidates or cfg["max_candidates"]
    label = cfg["label"].format(B=B, S=nsig, lo=snr[0], hi=snr[1], C=maxc)
    if args.traffic == "mixed":
        label = label.replace("CQ signals/frame", "signals/frame of MIXED traffic (not the headline recipe: ~22 % CQ calls, QSO messages of every type, duplicates)")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = world > 1 or args.force_dist
    if use_dist:
        # read by the HSA runtime when the process first touches the GPU (the decoder context is created before the process
        # group): the host driver of this pool only supports dmabuf IPC, without it RCCL fails with hipIpcGetMemHandle errors
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # the watchdog child exists before this process imports torch or touches the GPU (multi-rank / forced-dist runs only)
    wd = RankWatchdog(rank, world, use_dist, args.dist_timeout)
    hang, hang_limit = _hang_spec(args.test_hang)

    def enter(phase, timeout=None):
        if hang and hang == (rank, phase):
            wd.phase(phase, hang_limit or timeout)
            time.sleep(10 ** 7)                  # test hook: what a rank stuck inside a library call looks like from outside
        wd.phase(phase, timeout)

    enter("import_torch", max(args.dist_timeout, 600.0))        # the first import on a fresh box pages the image in: minutes
    import datetime
    import torch
    import torch.distributed as dist
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload

    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch as `python bench.py --gpus {args.gpus}` (self-launching) "
                         f"or through torch.distributed.run with --nproc-per-node {args.gpus}")
    if args.config == 1 and world != 1:
        raise SystemExit("--config 1 (CPU LDPC) is a single-GPU configuration")
    if args.backend == "gloo" and not args.dry:
        raise SystemExit("--backend gloo is only meaningful with --dry (the product path has no CPU form)")
    if args.dump_outputs and args.dry:
        raise SystemExit("--dump-outputs writes what the decode path computed: --dry runs none")
    total = B * world
    lo, hi = workload.shard_range(total, rank, world)
    assert hi - lo == B
    out = {
        "metric": METRIC, "value": None, "unit": "frames/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": label, "frames_per_gpu": B, "global_frames": total, "parallelism": f"frame-sharded x{world}"},
    }
    pg_timeout = datetime.timedelta(seconds=args.dist_timeout)
    ctl = {"store": None}                        # the process group's c10d store once it exists: rank diagnostics travel through it, not through RCCL

    def default_store():
        try:
            from torch.distributed import distributed_c10d
            return distributed_c10d._get_default_store()
        except Exception:
            return None

    def die(exc, extra=None):
        """a rank that fails after start-up leaves ONE diagnosable JSON line and a non-zero status; no clean shutdown of a broken group"""
        import traceback
        traceback.print_exc()
        if rank == 0 and out.get("value") is not None:
            # the timed region was complete and reduced: the measurement stands, the error is reported beside it
            out.update({"completed": False, "error_after_timing": f"{type(exc).__name__}: {exc}"[:1000], "error_phase": wd.current})
            emit(json.dumps(out))
        else:
            emit(failure_line(out, rank, world, wd.current, exc, ctl["store"], extra))
        wd.done()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(4)

    if args.dry:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()) if world == 1 else "29533")
        try:
            if world > 1:
                enter("init_process_group")
                dist.init_process_group(args.backend if args.backend == "gloo" else "gloo", rank=rank, world_size=world, timeout=pg_timeout)
                ctl["store"] = default_store()
                out["rccl_ranks"] = None
                out["backend"] = "gloo"
                out["ranks"] = dist.get_world_size()
                enter("rank_info")
                if ctl["store"] is not None:
                    store_publish(ctl["store"], f"ft8/info/{rank}", rank_info(torch, local_rank, False))
            enter("exchange_steps")
            ok = run_dry(args, out, rank, world, B, total, lo, hi, ctl["store"])
            if world > 1 and rank == 0 and ctl["store"] is not None:
                out["ranks_info"] = store_collect(ctl["store"], "ft8/info/", world, wait_s=10.0)
                out["per_rank_decode_only"] = store_collect(ctl["store"], "ft8/decode_only/", world, wait_s=10.0)
            enter("shutdown")
            if world > 1:
                dist.barrier()                   # rank 0 has read every rank's entries before the store's host may go away
                dist.destroy_process_group()
        except Exception as e:                   # noqa: BLE001 -- whatever it is, say where and exit non-zero
            die(e)
        wd.done()
        if rank == 0:
            emit(json.dumps(out))
        raise SystemExit(0 if ok else 1)

    enter("create_context")
    ndev = torch.cuda.device_count()
    if local_rank >= ndev:
        raise SystemExit(f"rank {rank}: local rank {local_rank} has no GPU ({ndev} visible); --gpus must not exceed the GPUs of the node")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # The decoder context -- and with it its three streams -- is created BEFORE the process group and before any torch
    # stream: HIP hands streams to a few hardware queues in creation order, and the pipeline needs its main and its two side
    # streams on three different queues.  (Created after RCCL's and torch's streams, the main and one side stream landed
    # on the same queue and the heap replay of part A no longer ran beside the waterfall of part B: +0.27 ms per step,
    # tools/trace_gaps.py on a rocprofv3 kernel trace.)
    # a stale or foreign libft8gpu.so fails here instead of producing numbers: the id baked into the library at link time must
    # be the one the sources beside it hash to
    out["build_id"] = ft8.check_build_id()

    def make_decoder():
        lib = None
        if args.ab_lib:
            lib = ft8.load_ab_library()
            out["library"] = "libft8gpu_ab.so (A/B build: not the shipped library) " + ft8.build_id(lib)
        d = ft8.Decoder(device=local_rank, max_frames=B, min_score=10, max_candidates=maxc, ldpc_iters=20, lib=lib)
        if args.debug_flags:
            d.set_debug_flags(args.debug_flags)
            out["debug_flags"] = args.debug_flags           # not the product configuration
        # the context has measured whether its streams co-run (ft8gpu_overlap_active): the two-part pipeline or the plain one
        out["overlap"] = d.overlap_active()
        if not out["overlap"]:
            out["overlap_reason"] = d.overlap_reason()
        return d

    dec = None
    single_ctx = not (args.config == 3 and world == 1)
    if single_ctx and not args.ctx_last:
        dec = make_decoder()
    decode_only = None
    if use_dist and dec is not None:
        # Before RCCL exists: this rank's decode rate with no collective anywhere near it (frames synthesised here are the
        # job's frames).  Should the process group or a collective fail later, every rank's figure is still known.
        enter("decode_only_warmup")
        try:
            _, tones0 = workload.message_pool(traffic=args.traffic)
            sig0, _ = workload.frame_signals(lo, B, nsig, tones0, snr_range=snr, dup_fraction=workload.MIXED_DUP_FRACTION if args.traffic == "mixed" else 0.0)
            iq0 = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device=dev)
            dec.synth_frames(sig0, B, nsig, 1.0, workload.SEED_BASE, iq0, first_frame=lo)
            s0 = torch.zeros((B, 1400), dtype=torch.uint8, device=dev)
            n0 = torch.zeros((B,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for _ in range(args.prewarm + 2):
                dec.decode_batch_dev(iq0, B, s0, n0)
            dec.synchronize()
            t = time.perf_counter()
            for _ in range(5):
                dec.decode_batch_dev(iq0, B, s0, n0)
            dec.synchronize()
            dt = (time.perf_counter() - t) / 5
            decode_only = {"ms_per_step": round(1e3 * dt, 4), "frames_per_s": round(B / dt, 1), "messages_per_frame": round(float(n0.float().mean().item()), 2),
                           "what": f"{B} frames per step on this rank's GPU, 5 steps, before the process group exists"}
            del iq0, s0, n0
        except Exception as e:                   # noqa: BLE001
            die(e)
    try:
        if use_dist:
            enter("init_process_group")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=pg_timeout)
            ctl["store"] = default_store()
            out["rccl_ranks"] = dist.get_world_size()          # what RCCL itself was initialised with
            out["backend"] = dist.get_backend()
            enter("rank_info")
            if ctl["store"] is not None:
                store_publish(ctl["store"], f"ft8/info/{rank}", rank_info(torch, local_rank, True))
                if decode_only:
                    store_publish(ctl["store"], f"ft8/decode_only/{rank}", decode_only)
            enter("first_collective")                           # RCCL builds its rings / proxies on the first call, not at init
            probe = torch.full((1,), float(rank), dtype=torch.float32, device=dev)
            dist.all_reduce(probe)
            torch.cuda.synchronize()
            if abs(float(probe.item()) - world * (world - 1) / 2) > 1e-3:
                raise RuntimeError(f"first all-reduce returned {float(probe.item())}, expected {world * (world - 1) / 2}")
    except Exception as e:                       # noqa: BLE001
        die(e, {"decode_only": decode_only})
    if single_ctx and args.ctx_last:
        held = [torch.cuda.Stream(device=dev) for _ in range(6)]       # what a framework would have created by now
        for st in held:
            with torch.cuda.stream(st):
                torch.zeros(1, device=dev)
        torch.cuda.synchronize()
        dec = make_decoder()
        out["ctx_created_last"] = True

    if args.config == 3 and world == 1:
        run_config3_one_gpu(args, out, B, nsig, snr, maxc, dev)
        wd.done()
        emit(json.dumps(out))
        return

    # The decoder keeps its OWN stream (its main / side streams are created together and sit on distinct hardware
    # queues; on a borrowed torch stream the same pipeline measured 1.48 instead of 1.28 ms at 1024 frames, cap 480).
    # torch sees that stream as an ExternalStream (events, waits); the RCCL gather is issued from a torch stream that
    # waits for the decoder's stream first, and the decoder waits for that stream before it rewrites a buffer.
    stream = torch.cuda.ExternalStream(dec.stream_handle(), device=dev)
    coll_stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(coll_stream)

    # ---- synthetic frames, generated in HBM (not timed); global frame g is the same samples for any world size
    enter("synth")
    _, pool_tones = workload.message_pool(traffic=args.traffic)
    sig, _ = workload.frame_signals(lo, B, nsig, pool_tones, snr_range=snr,
                                    dup_fraction=workload.MIXED_DUP_FRACTION if args.traffic == "mixed" else 0.0)
    iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device=dev)
    dec.synth_frames(sig, B, nsig, 1.0, workload.SEED_BASE, iq, first_frame=lo)
    out["config"]["traffic"] = args.traffic

    if args.config == 1:
        run_config1(args, out, dec, iq, B, maxc, stream, dev)
        dec.close()
        wd.done()
        emit(json.dumps(out))
        return

    # spot records: two buffers per rank; the exchange of step k (one asynchronous RCCL all-gather of
    # records + counts) runs under the kernels of step k + 1 and is drained inside the timed region
    exchange = use_dist and not args.no_exchange
    exch = workload.SpotExchange(B, world, dev, collective=exchange)
    if use_dist:
        out["exchange"] = "one asynchronous all_gather_into_tensor of records + counts per step" if exchange else \
            "none (--no-exchange control leg: no collective in the step; barrier + timing reduction only)"
    torch.cuda.synchronize()                            # the buffers were zero-filled on torch's stream
    spots, nres = exch.buffers(0)
    state = {"k": 0}
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    fail = _rank_step(args.test_fail_exchange)

    def step():
        k = state["k"]
        s_buf, n_buf = exch.buffers(k)                  # (the collective stream) waits for the exchange that last used this buffer
        if exchange:
            stream.wait_stream(coll_stream)             # ... and the decoder for the collective stream
        dec.decode_batch_dev(iq, B, s_buf, n_buf)
        if exchange:
            coll_stream.wait_stream(stream)             # the gather is ordered behind the kernels that produce the records
        if fail and fail == (rank, str(k)):
            raise RuntimeError(f"simulated collective failure at step {k} (--test-fail-exchange)")
        exch.launch(k)                                  # the whole job's spot list on every rank
        state["k"] = k + 1

    def fence():
        exch.wait_all()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    try:
        # the clock / power sampler (--full) starts before the warm-up so that its thread start-up does not land in the first timed step
        with ClockSampler(local_rank, args.full and not args.no_clock_sampler) as clk:
            enter("warmup_with_exchange" if exchange else "warmup")
            n_pre = args.prewarm
            for _ in range(args.prewarm):
                step()
            if args.prewarm_seconds > 0:
                fence()
                t_cal = time.perf_counter()
                for _ in range(8):
                    step()
                fence()
                extra = int(min(5000, np.ceil(args.prewarm_seconds / max((time.perf_counter() - t_cal) / 8, 1e-4))))
                if use_dist:                     # the exchange is a collective: every rank runs the same number of steps
                    nmax = torch.tensor([extra], dtype=torch.int64, device=dev)
                    dist.all_reduce(nmax, op=dist.ReduceOp.MAX)
                    extra = int(nmax.item())
                for i in range(extra):
                    step()
                    if (i & 127) == 127:
                        exch.wait_all()
                        torch.cuda.synchronize()
                n_pre += 8 + extra
            for _ in range(args.warmup):
                step()
            fence()
            enter("timed_steps", args.dist_timeout + 60.0)
            if args.full:
                dec.enable_timing(True)      # stage events are recorded on the stream, read after the fence
            clk.clear()
            t0 = time.perf_counter()
            step_ev[0].record(stream)
            for i in range(args.steps):
                step()
                step_ev[i + 1].record(stream)   # per-step spread: decode kernels of step i (the exchange runs on RCCL's stream)
            if use_dist:
                # where a multi-rank step's time goes: this rank's kernels are done at t_kernels; whatever the fence still
                # waits for after that is the exposed tail of the last gathers plus the skew between the ranks (the barrier)
                stream.synchronize()
                t_kernels = time.perf_counter() - t0
            fence()
            elapsed = time.perf_counter() - t0
        if args.full:
            stage_avg = dec.timings()    # mean over the timed steps (ring of the last 32)
            timed_runs = stage_avg.pop("runs")
            dec.enable_timing(False)
        spots, nres = exch.buffers(state["k"] - 1) if state["k"] > 0 else (spots, nres)    # the last step's local records
        per_step = [step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(args.steps)]

        enter("reduce_timings")
        my_elapsed = elapsed
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if use_dist:
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        if use_dist:
            # per-rank view of the same timed region (one small all-gather, after the clock): which rank is slow, whether its
            # context runs the overlapped pipeline, how long its own kernels took and what the gather drain + barrier added
            mine = torch.tensor([my_elapsed, t_kernels, my_elapsed - t_kernels, 1.0 if out.get("overlap") else 0.0, float(np.median(per_step))],
                                dtype=torch.float64, device=dev)
            every = torch.empty(world * mine.numel(), dtype=torch.float64, device=dev)
            dist.all_gather_into_tensor(every, mine)
            every = every.view(world, -1).cpu().numpy()
            ms = 1e3 * every[:, 0] / args.steps
            out["ranks_detail"] = {
                "ms_per_step": [round(float(v), 4) for v in ms], "ms_per_step_min": round(float(ms.min()), 4), "ms_per_step_max": round(float(ms.max()), 4),
                "imbalance": round(float(ms.max() / ms.min() - 1.0), 5),
                "kernels_done_ms_per_step": [round(1e3 * float(v) / args.steps, 4) for v in every[:, 1]],
                "exposed_gather_drain_and_barrier_ms_total": [round(1e3 * float(v), 4) for v in every[:, 2]],
                "overlap": [bool(v) for v in every[:, 3]], "median_step_kernels_ms": [round(float(v), 4) for v in every[:, 4]],
                "note": "per rank, same timed region: wall per step; host time until the rank's own kernels were done; what the final fence (gather "
                        "drain + barrier) added once, after them; ft8gpu_overlap_active of the rank's context; median hipEvent step time"}
            if rank == 0 and ctl["store"] is not None:
                # first-contact facts, through the c10d store (TCP): RCCL version, what each rank sees and which physical GPU it holds,
                # and each rank's decode-only rate measured before RCCL existed (decode scaling without any collective nearby)
                out["ranks_info"] = store_collect(ctl["store"], "ft8/info/", world, wait_s=10.0)
                out["per_rank_decode_only"] = store_collect(ctl["store"], "ft8/decode_only/", world, wait_s=10.0)
                rates = [v.get("frames_per_s") for v in out["per_rank_decode_only"].values() if v.get("frames_per_s")]
                if rates:
                    out["decode_only_frames_per_s_sum"] = round(float(sum(rates)), 1)

        out["value"] = round(total * args.steps / elapsed, 1)
        out["ms_per_step"] = round(1e3 * elapsed / args.steps, 3)
        if rank == 0:
            wd.result(out)               # from here on a hang or an error costs diagnostics, not the measurement (see RankWatchdog.result, die)
        out["step_ms"] = {"min": round(min(per_step), 4), "median": round(float(np.median(per_step)), 4), "max": round(max(per_step), 4),
                          "slowest_step_index": int(np.argmax(per_step)),
                          "note": "hipEvent time between consecutive steps' last kernels on rank 0's stream"}
        out["prewarm_steps"] = n_pre               # untimed, before the W warm-up steps (clock settling after idle; see --prewarm-seconds)
        out["prewarm_seconds"] = args.prewarm_seconds
        if args.dump_outputs and rank == 0:
            # what a caller receives from the last timed step: the whole job's gathered list where there is one, else the local records
            rs, rc = exch.gathered(state["k"] - 1) if exchange and world > 1 else (spots, nres)
            out["dumped_outputs"] = dump_outputs(args.dump_outputs, rs.cpu().numpy(), rc.cpu().numpy())
        if args.full:
            out["gpu_clock"] = clk.summary()
            if (out["gpu_clock"] or {}).get("power_w_median"):
                # hwmon's socket power is a moving average with a time constant of a fraction of a second: over a timed region of
                # K x 4 ms that follows 0.1 s of warm-up from idle it still reads hundreds of watts low (round 5 quoted 889 W from here;
                # a 60 s run of the same loop reads 1 380 W, --sustain-seconds).  Energy per frame is therefore reported there only.
                out["gpu_clock"]["power_note"] = "moving average, lags a burst this short: read sustained.power_w (--sustain-seconds) for the power this loop draws"
            out["config"]["decoded_messages_per_frame"] = round(float(nres.cpu().numpy().mean()), 2)
            # slots the path wrote (messages whose first token starts with "CQ", rtlsdr_ft8d.c:1509-1519); the other messages are
            # counted in n_results and leave their slot as the caller's array had it (zeros here)
            rec = spots.view(B, ft8.MAX_MESSAGES, 28)
            used = torch.arange(ft8.MAX_MESSAGES, device=dev)[None, :] < nres[:, None]
            out["config"]["cq_spots_per_frame"] = round(float(((rec != 0).any(dim=2) & used).sum().item()) / B, 2)
        if rank == 0:
            wd.result(out)
        if exchange and world > 1:
            # the gathered list of the last step must hold every rank's records in global frame order (this block first runs on the
            # first node with two GPUs: whatever it does, the measurement above stands)
            try:
                gs, gc = exch.gathered(state["k"] - 1)
                mine = bool(torch.equal(gs[lo:hi], spots)) and bool(torch.equal(gc[lo:hi], nres))
                flag = torch.tensor([1 if mine else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                out["gathered_list_holds_every_ranks_shard"] = bool(flag.item())
                out["config"]["gathered_messages_per_frame"] = round(float(gc.float().mean().item()), 2)
            except Exception as e:               # noqa: BLE001
                out["gathered_list_check_error"] = f"{type(e).__name__}: {e}"[:500]
            if rank == 0:
                wd.result(out)
        if args.sustain_seconds > 0:
            # a side figure, never the headline: the same loop for S seconds (step count fixed from the all-reduced step time,
            # so every rank runs the same number of collectives)
            n_sus = max(64, int(np.ceil(args.sustain_seconds * 1e3 / (1e3 * elapsed / args.steps))))
            enter("sustained", args.dist_timeout + 3.0 * args.sustain_seconds + 60.0)
            try:
                sus = run_sustained(args, torch, dist, step, fence, stream, local_rank, n_sus, B, world, use_dist, dev, 1e3 * elapsed / args.steps)
                if rank == 0:
                    out["sustained"] = sus
            except Exception as e:               # noqa: BLE001 -- a side figure: its failure must not take the headline with it
                out["sustained_error"] = f"{type(e).__name__}: {e}"[:500]
    except Exception as e:                       # noqa: BLE001
        if not use_dist:
            raise
        die(e, {"decode_only": decode_only, "steps_launched": state["k"]})
    enter("report", max(args.dist_timeout, 600.0))
    if rank == 0 and args.full:
        launches = int(stage_avg.pop("launches_per_stage", 1))
        kernels = {k: v for k, v in stage_avg.items() if k != "total_ms"}
        dom = max(kernels, key=kernels.get)
        dom_ms = kernels[dom]
        name = dom.replace("_ms", "")
        achieved = BYTES_PER_FRAME * B / (dom_ms * 1e-3) / 1e9
        pmc = pmc_figures(name, B, launches, dom_ms / launches, args.config)
        valu_bound = name == "decode"
        out["roofline"] = {
            # the contract's figure: algorithmic bytes of the launch / the dominant kernel's duration, against HBM.
            # The dominant kernel (LDPC BP) is bound by VALU issue, not by HBM: `bound` names what binds it, the
            # HBM fraction the contract asks for stays in achieved / peak / frac (= hbm_frac)
            "bound": "valu" if valu_bound else "hbm", "kernel": name, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS,
            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 5), "hbm_frac": round(achieved / HBM_PEAK_GBPS, 5),
            "traffic": pmc.get("traffic"),
            "binding_resource": "valu-issue" if valu_bound else None,
            "valu_busy_frac_pmc": pmc.get("valu_busy"), "valu_busy_frac_pmc_raw": pmc.get("valu_busy_raw"),
            "valu_frac_of_fp32_peak_pmc": pmc.get("valu_frac"),
            "kernel_hbm_GBps_from_traffic": pmc.get("kernel_hbm_GBps"), "pmc_from": pmc.get("pmc_from"),
            "pmc_pipeline_form": pmc.get("pmc_pipeline_form"),
            "frac_of_measured_copy_peak": round(achieved / HBM_COPY_PEAK_GBPS, 5),
            "kernel_ms": round(dom_ms, 4), "kernel_launches_per_step": launches,
            "kernel_ms_per_launch": round(dom_ms / launches, 4), "algorithmic_bytes_per_launch": BYTES_PER_FRAME * B // launches,
            "stage_ms": {k: round(v, 4) for k, v in stage_avg.items()}, "stage_ms_runs": timed_runs,
            "pipeline_achieved_GBps": round(BYTES_PER_FRAME * B / (stage_avg["total_ms"] * 1e-3) / 1e9, 2),
            # every kernel against the HBM roof on ITS OWN algorithmic bytes (what it must read and write once):
            # waterfall 384 000 B of IQ in + 94 208 B out; sync the 94 208 B waterfall in + the survivor lists out (about 1.5 KB);
            # decode the waterfall cells its candidates gather (58 symbols x 8 tones x 114 candidates, at most the 94 208 B) + 48 B
            # records; spots the records in + 1 404 B out.  Only the waterfall kernel is anywhere near a bandwidth bound.
            "per_kernel": {k: {"own_bytes_per_frame": b, "ms": round(stage_avg[k + "_ms"], 4),
                               "GBps": round(b * B / (stage_avg[k + "_ms"] * 1e-3) / 1e9, 1),
                               "frac_of_hbm_peak": round(b * B / (stage_avg[k + "_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)}
                           for k, b in (("waterfall", 384000 + 94208), ("sync", 94208 + 1536), ("decode", 94208 + 114 * 48), ("spots", 114 * 48 + 1404))
                           if stage_avg.get(k + "_ms", 0) > 0},
        }
        if world == 1 and not args.no_cpu_baseline and args.cpu_frames > 0:
            out["cpu_baseline"] = cpu_baseline(iq, spots, nres, min(args.cpu_frames, B), maxc)
        if world == 1 and not args.no_host_legs:
            out["end_to_end"] = host_legs(dec, iq, spots, nres, B)
    dec.close()
    if use_dist:
        enter("shutdown")
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception as e:                   # noqa: BLE001 -- the numbers exist: report them, and the shutdown trouble beside them
            out["shutdown_error"] = f"{type(e).__name__}: {e}"[:500]
    wd.done()
    if rank == 0:
        sys.stdout.flush()
        sys.stderr.flush()
        try:                                        # RCCL writes its banner through C stdio, which is fully buffered
            import ctypes                           # on a pipe: push it out before the JSON line, not at exit
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        emit(json.dumps(out))          # the one JSON line, after any library banners


def run_config3_one_gpu(args, out, B, nsig, snr, maxc, dev):
    """configs[3] when only one GPU is there: the 32768-frame job as `--shards` contiguous shards of B frames, each with
    its own context (own streams and HBM buffers) on this GPU, decoded through the C multi-GPU entry
    ft8gpu_decode_batch_multi_dev (one host thread per shard, records gathered at their frame offsets on the host).
    On an 8-GPU node the same job is `--gpus 8` (one shard per GPU, RCCL gather)."""
    import torch
    import rtlsdr_ft8d_amd as ft8
    from rtlsdr_ft8d_amd import workload
    S = args.shards
    total = S * B
    _, pool_tones = workload.message_pool(traffic=args.traffic)
    out["config"]["traffic"] = args.traffic
    decs, iqs = [], []
    for g in range(S):
        d = ft8.Decoder(device=dev.index, max_frames=B, min_score=10, max_candidates=maxc, ldpc_iters=20)
        lo, hi = workload.shard_range(total, g, S)
        sig, _ = workload.frame_signals(lo, B, nsig, pool_tones, snr_range=snr,
                                        dup_fraction=workload.MIXED_DUP_FRACTION if args.traffic == "mixed" else 0.0)
        iq = torch.empty((B, 2, ft8.NSAMPLES), dtype=torch.float32, device=dev)
        d.synth_frames(sig, B, nsig, 1.0, workload.SEED_BASE, iq, first_frame=lo)
        decs.append(d)
        iqs.append(iq)
    decodes = np.zeros((total, ft8.MAX_MESSAGES), ft8.RESULT_DTYPE)
    n = None
    for _ in range(max(args.warmup, 1)):
        decodes, n = ft8.decode_batch_multi_dev(decs, iqs, [B] * S, decodes)
    torch.cuda.synchronize()
    per_step = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        t1 = time.perf_counter()
        decodes, n = ft8.decode_batch_multi_dev(decs, iqs, [B] * S, decodes)       # returns with the records on the host
        per_step.append(1e3 * (time.perf_counter() - t1))
    elapsed = time.perf_counter() - t0
    out["value"] = round(total * args.steps / elapsed, 1)
    out["ms_per_step"] = round(1e3 * elapsed / args.steps, 3)
    if args.dump_outputs:
        out["dumped_outputs"] = dump_outputs(args.dump_outputs, decodes, n)
    out["step_ms"] = {"min": round(min(per_step), 3), "median": round(float(np.median(per_step)), 3), "max": round(max(per_step), 3)}
    out["config"].update({"global_frames": total, "shards": S, "parallelism": f"{S} contexts on one GPU, host threads, host-side gather (D2H of the records inside the step)",
                          "decoded_messages_per_frame": round(float(n.mean()), 2)})
    # the same frames, shard by shard through ONE context: records must be identical
    same = 0
    spots = torch.zeros((B, 1400), dtype=torch.uint8, device=dev)
    nres = torch.zeros((B,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                 # the fills run on torch's stream, the decoder on its own
    for g in range(S):
        spots.zero_()                        # bytes behind the NUL of call / loc are never written: same start as `decodes`
        torch.cuda.synchronize()
        decs[0].decode_batch_dev(iqs[g], B, spots, nres)
        decs[0].synchronize()
        a = spots.cpu().numpy().view(ft8.RESULT_DTYPE).reshape(B, ft8.MAX_MESSAGES)
        c = nres.cpu().numpy()
        for k in range(B):
            m = min(int(c[k]), ft8.MAX_MESSAGES)
            same += int(c[k] == n[g * B + k] and a[k, :m].tobytes() == decodes[g * B + k, :m].tobytes())
    out["config"]["frames_identical_to_single_context_walk"] = f"{same}/{total}"
    out["roofline"] = {"bound": "valu", "kernel": "decode", "achieved": round(BYTES_PER_FRAME * total / (elapsed / args.steps) / 1e9, 2),
                       "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(BYTES_PER_FRAME * total / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBPS, 5),
                       "traffic": None, "note": "whole-step figure (8 overlapping contexts: no per-kernel events); see --config 2 for the per-kernel roofline"}
    for d in decs:
        d.close()


def run_config1(args, out, dec, iq, B, maxc, stream, dev):
    """configs[1]: waterfall + sync (+ exact heap) on the GPU, results to the host, LDPC on the host cores"""
    import torch
    import rtlsdr_ft8d_amd as ft8
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    oracle_lib.lib()
    cores = usable_cores()
    p = oracle_lib.default_params(10, maxc, 20)
    mag = torch.empty((B, ft8.MAG_ARRAY), dtype=torch.uint8, device=dev)
    cands = torch.empty((B, maxc, 8), dtype=torch.uint8, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    h_mag = torch.empty((B, ft8.MAG_ARRAY), dtype=torch.uint8).pin_memory()
    h_cands = torch.empty((B, maxc, 8), dtype=torch.uint8).pin_memory()
    h_counts = torch.empty((B,), dtype=torch.int32).pin_memory()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    acc = {"waterfall_ms": 0.0, "sync_heap_ms": 0.0, "d2h_ms": 0.0, "cpu_ldpc_ms": 0.0}
    res = {}

    def step(timed):
        ev[0].record(stream)
        dec.waterfall_dev(iq, B, mag)
        ev[1].record(stream)
        dec.find_sync_dev(mag, B, cands, counts)
        ev[2].record(stream)
        cur = torch.cuda.current_stream(dev)            # the copies run on torch's stream, behind the decoder's kernels
        cur.wait_stream(stream)
        h_mag.copy_(mag, non_blocking=True)
        h_cands.copy_(cands, non_blocking=True)
        h_counts.copy_(counts, non_blocking=True)
        ev[3].record(cur)
        cur.synchronize()
        t = time.perf_counter()
        res["dec"], res["n"] = oracle_lib.decode_from_candidates_batch(
            h_mag.numpy(), h_cands.numpy().view(oracle_lib.CAND_DTYPE).reshape(B, maxc), h_counts.numpy(), p, cores)
        if timed:
            acc["cpu_ldpc_ms"] += 1e3 * (time.perf_counter() - t)
            acc["waterfall_ms"] += ev[0].elapsed_time(ev[1])
            acc["sync_heap_ms"] += ev[1].elapsed_time(ev[2])
            acc["d2h_ms"] += ev[2].elapsed_time(ev[3])

    for _ in range(args.warmup):
        step(False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    stage = {k: v / args.steps for k, v in acc.items()}
    out["value"] = round(B * args.steps / elapsed, 1)
    out["ms_per_step"] = round(1e3 * elapsed / args.steps, 3)
    if args.dump_outputs:
        out["dumped_outputs"] = dump_outputs(args.dump_outputs, res["dec"], res["n"])
    # BASELINE configs[1] asks for "LDPC on CPU"; the product has no CPU LDPC, so that half is the test oracle and this
    # `value` is bound by it: it is NOT a product rate.  The product's share is roofline.gpu_part_frames_per_s.
    out["value_is_product"] = False
    out["value_bound_by"] = "oracle-bound: the host LDPC half of every step is the CPU oracle (test infrastructure)"
    out["config"]["decoded_messages_per_frame"] = round(float(res["n"].mean()), 2)
    out["config"]["host_cores_for_ldpc"] = cores
    gpu_ms = stage["waterfall_ms"] + stage["sync_heap_ms"] + stage["d2h_ms"]
    dom_ms = stage["waterfall_ms"]
    achieved = BYTES_PER_FRAME_CFG1 * B / (dom_ms * 1e-3) / 1e9
    pmc = pmc_figures("waterfall", B, 1, dom_ms, 1)
    out["roofline"] = {"bound": "hbm", "kernel": "waterfall", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                       "frac": round(achieved / HBM_PEAK_GBPS, 5), "traffic": pmc.get("traffic"), "valu_busy_frac_pmc": pmc.get("valu_busy"),
                       "kernel_hbm_GBps_from_traffic": pmc.get("kernel_hbm_GBps"), "pmc_from": pmc.get("pmc_from"), "kernel_ms": round(dom_ms, 4),
                       "algorithmic_bytes_per_launch": BYTES_PER_FRAME_CFG1 * B,
                       "stage_ms": {k: round(v, 4) for k, v in stage.items()},
                       "gpu_part_frames_per_s": round(B / (gpu_ms * 1e-3), 1),
                       "note": "the step time is the host LDPC; the GPU part (waterfall + sync + heap + D2H) alone would run at gpu_part_frames_per_s"}
    # the same frames through the all-GPU path must give the same records
    gd, gn = dec.decode_batch(iq.cpu().numpy())
    same = sum(int(gn[k] == res["n"][k] and gd[k].tobytes() == res["dec"][k].tobytes()) for k in range(B))
    out["cpu_baseline"] = {"value": round(B / (stage["cpu_ldpc_ms"] * 1e-3), 2), "unit": "frames/s", "cores": cores, "kind": "port",
                           "sample": f"the LDPC half of every step: oracle ft8o_decode_from_candidates_batch on {B} frames, OpenMP {cores} threads",
                           "identical_to_all_gpu_path": f"{same}/{B}"}


def pmc_figures(kernel, frames, launches, ms_per_launch, config=2):
    """PMC-derived figures of the dominant kernel from the committed rocprofv3 summaries (profiles/pmc_traffic.json,
    profiles/pmc_counters.json: FETCH_SIZE / WRITE_SIZE / SQ passes over this very command, tools/gpu_round.sh; the
    entries of configs[1] and configs[4] sit under "config1" / "config4").  They describe the kernel sources they were
    collected on: the summary carries a hash of csrc/ and the figures are reported only while it matches the tree this
    bench runs from (and the launch size); otherwise null."""
    none = {"traffic": None, "valu_busy": None, "valu_busy_raw": None, "valu_frac": None, "kernel_hbm_GBps": None, "pmc_from": None, "pmc_pipeline_form": None}
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return none
    # Per-frame figures carry over between the plain and the two-part pipeline only for the kernels that are the SAME code
    # in both: the heap replay is not (wave-per-frame kernel in the counted plain run, lane-per-frame kernel for part B of the
    # product run), so it gets no counter figures here.
    if kernel not in ("waterfall", "sync", "decode", "spots"):
        return none
    sect = t if config == 2 else t.get(f"config{config}", {})
    e = sect.get(kernel, {})
    if not e or "hbm_bytes_per_frame" not in e or t.get("csrc_sha") != csrc_hash():
        return none
    # The counter passes serialise kernels, so the context's co-execution probe selects the plain pipeline there (one
    # launch per stage and batch); per-frame figures are what carries over to this run's launches of frames // launches.
    per_launch = frames // launches
    traffic = int(round(e["hbm_bytes_per_frame"] * per_launch))
    insts = e.get("valu_instructions_per_frame")
    # SQ_ACTIVE_INST_VALU and SQ_BUSY_CYCLES come from two counter passes (two runs of the command): on a saturated VALU pipe the
    # quotient can read a hair above 1.  The fraction is reported clamped to 1.0, the raw quotient beside it.
    busy_raw = e.get("valu_busy_frac_raw", e.get("valu_busy_frac"))
    return {"traffic": traffic, "valu_busy": None if busy_raw is None else min(1.0, busy_raw), "valu_busy_raw": busy_raw,
            "valu_frac": round(insts * per_launch * 64 / (ms_per_launch * 1e-3) / FP32_VALU_PEAK, 4) if insts else None,
            "kernel_hbm_GBps": round(traffic / (ms_per_launch * 1e-3) / 1e9, 1),
            "pmc_from": f"profiles/pmc_traffic.json{'' if config == 2 else ' [config%d]' % config} @ csrc {t.get('csrc_sha')}"
                        f" (per-frame counters of {e.get('frames_per_launch')}-frame launches of the {t.get('pipeline_form', 'plain')} pipeline x {per_launch} frames)",
            "pmc_pipeline_form": t.get("pipeline_form", "plain")}


def usable_cores():
    """host cores this process may actually use: affinity mask capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                txt = f.read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, q // int(f.read())))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def cpu_baseline(iq, spots, nres, m, max_candidates):
    """The reference's path on the host cores, timed on the first m frames of the same batch, one frame per OpenMP task.
    The reference itself cannot be built here (ft8_lib submodule empty, no fftw3.h), so everything behind the FFT is
    the oracle's restatement either way.  The FFT is DETECTED, not assumed: when libfftw3f.so.3 is on the box the oracle
    binds it at run time and transforms as the reference does (fftwf_plan_dft_1d(1024, FFTW_FORWARD, FFTW_ESTIMATE),
    rtlsdr_ft8d.c:326; executed per row, :1411) -> kind "reference-fft", with the flips against the oracle's own radix-4
    FFT counted; otherwise kind "port" with the library names that were searched.  The same sample doubles as a parity
    check of the GPU results."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    import rtlsdr_ft8d_amd as ft8
    oracle_lib.lib()
    cores = usable_cores()
    host_iq = iq[:m].cpu().numpy()
    p = oracle_lib.default_params(10, max_candidates, 20)
    oracle_lib.subsystem_batch(host_iq[:min(m, cores)], p, cores)          # warm-up (page-in, thread pool)
    t0 = time.perf_counter()
    rdec, rn = oracle_lib.subsystem_batch(host_iq, p, cores)
    dt = time.perf_counter() - t0
    m1 = min(m, 64)
    t1 = time.perf_counter()
    oracle_lib.subsystem_batch(host_iq[:m1], p, 1)
    dt1 = time.perf_counter() - t1
    g_dec = spots[:m].cpu().numpy().view(ft8.RESULT_DTYPE).reshape(m, ft8.MAX_MESSAGES)
    g_n = nres[:m].cpu().numpy()
    same = sum(int(g_n[k] == rn[k] and g_dec[k].tobytes() == rdec[k].tobytes()) for k in range(m))
    port = {"value": round(m / dt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"first {m} frames of the bench batch through oracle ft8o_subsystem_batch (gcc -O3 -ffp-contract=off, the oracle's own radix-4 "
                      f"FFT, OpenMP {cores} threads), {dt:.2f} s wall",
            "single_core_frames_per_s": round(m1 / dt1, 2), "os_cpu_count": os.cpu_count(),
            "gpu_vs_oracle_identical_frames": f"{same}/{m}"}
    have_fftw, detail = oracle_lib.fftw_init(None)
    if not have_fftw:
        port["fftw3f"] = f"not found (searched: {detail})"
        return port
    oracle_lib.subsystem_batch_fftw(host_iq[:min(m, cores)], p, cores)
    t2 = time.perf_counter()
    fdec, fn = oracle_lib.subsystem_batch_fftw(host_iq, p, cores)
    dtf = time.perf_counter() - t2
    t3 = time.perf_counter()
    oracle_lib.subsystem_batch_fftw(host_iq[:m1], p, 1)
    dtf1 = time.perf_counter() - t3
    mw = min(m, 256)
    wf_fftw = oracle_lib.waterfall_batch(host_iq[:mw], 2, cores)
    wf_own = oracle_lib.waterfall_batch(host_iq[:mw], False, cores)
    same_f = sum(int(fn[k] == rn[k] and fdec[k].tobytes() == rdec[k].tobytes()) for k in range(m))
    return {"value": round(m / dtf, 2), "unit": "frames/s", "cores": cores, "kind": "reference-fft",
            "sample": f"first {m} frames of the bench batch: the reference's FFT (fftw3f bound at run time from {detail}: fftwf_plan_dft_1d 1024 FFTW_FORWARD "
                      f"FFTW_ESTIMATE, one fftwf_execute_dft per row) + the oracle's restatement of everything behind it, OpenMP {cores} threads, {dtf:.2f} s wall",
            "single_core_frames_per_s": round(m1 / dtf1, 2), "os_cpu_count": os.cpu_count(), "fftw3f": detail,
            "fft_flips_vs_own_radix4": {"waterfall_bytes_differing": int((wf_fftw != wf_own).sum()), "of_bytes": int(wf_own.size),
                                        "frames_with_different_records": m - same_f, "of_frames": m},
            "port_with_own_fft": port, "gpu_vs_oracle_identical_frames": f"{same}/{m}"}


def host_legs(dec, iq, spots, nres, B):
    """The PCIe-inclusive rates a replay user sees, beside the HBM-resident `value` (never instead of it):
    host_fed: ft8gpu_decode_batch on frames in (pinned) host memory, 384 KB/frame uploaded in 512-frame chunks
              on a copy stream under the kernels of the previous chunk, records copied back;
    rx_host_fed: ft8gpu_rx_decimate on raw 2.4 Msps u8 captures in host memory (72 MB per 15 s capture) followed
              by the decode of the frames it produces."""
    import torch
    out = {}
    m = min(B, 2048)
    import rtlsdr_ft8d_amd as ft8
    pinned = ft8.PinnedArray((m, 2, ft8.NSAMPLES), np.float32)           # ft8gpu_host_alloc: what a C caller of the host entries would use
    h = pinned.array
    h[...] = iq[:m].cpu().numpy()
    dec.decode_batch(h[:min(m, 512)])                                    # warm-up (staging allocation)
    t0 = time.perf_counter()
    d, n = dec.decode_batch(h)
    dt = time.perf_counter() - t0
    same = bool(np.array_equal(n, nres[:m].cpu().numpy())) and d.tobytes() == spots[:m].cpu().numpy().tobytes()
    out["host_fed_frames_per_s"] = round(m / dt, 1)
    out["host_fed"] = {"frames": m, "ms": round(1e3 * dt, 2), "upload_GBps": round(m * 384000 / dt / 1e9, 1), "records_identical_to_hbm_resident_run": same,
                       "host_memory": "ft8gpu_host_alloc (page-locked)"}
    del h                                                                # no view may outlive the allocation (PinnedArray.close refuses)
    pinned.close()
    ncap, npairs = 4, 36_000_000                                         # 15 s at 2.4 Msps
    raw = torch.randint(0, 256, (ncap, 2 * npairs), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).pin_memory().numpy()
    dec.rx_decimate(raw)                                                 # warm-up at full size (staging buffers are grown on first use)
    t0 = time.perf_counter()
    frames = dec.rx_decimate(raw)
    t1 = time.perf_counter()
    dec.decode_batch(frames)
    t2 = time.perf_counter()
    out["rx_host_fed_captures_per_s"] = round(ncap / (t2 - t0), 2)
    # the daemon's operating point: ONE frame per 15 s slot through the drop-in ft8_subsystem (rtlsdr_ft8d.h:164),
    # host pointers in and out, process-global single-frame context (the median of 50 calls; the first call creates it)
    one = iq[0].cpu().numpy()
    i_s, q_s = np.ascontiguousarray(one[0]), np.ascontiguousarray(one[1])
    ft8.ft8_subsystem(i_s, q_s)
    lat = []
    for _ in range(50):
        t3 = time.perf_counter()
        d1, n1 = ft8.ft8_subsystem(i_s, q_s)
        lat.append(1e3 * (time.perf_counter() - t3))
    m1 = min(int(n1), ft8.MAX_MESSAGES)
    ref1 = spots[0].cpu().numpy().view(ft8.RESULT_DTYPE)
    out["single_frame_ms"] = round(float(np.median(lat)), 4)
    out["single_frame"] = {"entry": "ft8_subsystem (drop-in, one 15 s frame, host buffers)", "median_ms": round(float(np.median(lat)), 4),
                           "min_ms": round(min(lat), 4), "max_ms": round(max(lat), 4), "calls": len(lat),
                           "records_identical_to_batch_run": bool(n1 == int(nres[0].item()) and d1[:m1].tobytes() == ref1[:m1].tobytes())}
    out["rx_host_fed"] = {"captures": ncap, "raw_bytes_per_capture": 2 * npairs, "decimate_ms": round(1e3 * (t1 - t0), 2),
                          "decode_ms": round(1e3 * (t2 - t1), 2), "upload_GBps": round(ncap * 2 * npairs / (t1 - t0) / 1e9, 1)}
    return out


if __name__ == "__main__":
    main()
