#!/usr/bin/env python3
"""bench.py -- GElem/s of the LSQ fake-quantize hot path (forward op + backward op) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2|cfg1|cfg3|cfg4|cfg5|cfg5_bf16|cfg5_axis0|tok|tok_bf16|vit|vit_bf16|
                                                                        cfg2_misaligned|cfg5[_bf16]_misaligned|cfg5[_bf16]_channels_last|cfg5[_bf16]_mixed_layout]

One "step" = one forward op + one backward op (training mode) over one batch of synthetic input already resident
in HBM.  The default workload is BASELINE.json config 2 -- per-tensor quint8, fp32 [128,512,56,56] (205.5 M elements,
822 MB per tensor) PER GPU; the per-channel half of the path has its own workloads (cfg3, cfg5, cfg5_bf16).

`--gpus N` with N > 1: when the process was not started by a launcher (no WORLD_SIZE in the environment) bench.py
starts the N ranks itself -- fresh child processes, one per GPU, created before anything in this process touches the
GPU -- and exits non-zero if fewer than N devices are visible; it never degrades to a smaller run.  Under
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` it is one of the ranks.  With N > 1 the batch
is sharded across the ranks (weak scaling: every rank owns a full-size shard; `--workload cfg4` is the strong-scaled
[1024,1024,14,14] / N), the backward uses the GLOBAL element count in the gradient scaler and ONE RCCL all-reduce of the
packed fp64 [d_scale, d_shift] sums per step -- inside the timed region.

Workloads that stream less than 1 GiB per step (everything but config 2 and a config-4 shard at small N) rotate through
`config.input_buffer_sets` copies of (x, grad), more than 1 GiB of inputs in total, the backward working on a set the
forward last touched half a rotation ago: otherwise the part's 256 MB Infinity Cache serves a config-5-sized step and the
"HBM" fraction is not one (DESIGN_HISTORY.md section 7).  `--buffers 1` re-uses one set.

Rank 0 prints ONE JSON line; `value` is the whole-job aggregate: (elements of all ranks * K) / time,
time = max over ranks of the K-step wall time bracketed by barrier + synchronize; `ms_per_step` is that time / K.

`--dump-outputs DIR` writes what the headline's last timed step returned -- y, dx, d_scale, d_shift -- as DIR/<name>.npy (float32;
float64 storage: float64), at most 64 MB in all: outputs too large for that are sampled at fixed, seeded positions.  The
inputs are seeded (torchlsq.synth), so two builds run with the same arguments can be compared output for output.

A plain run does only what that line needs: it sets up, warms up, times the K steps, writes --dump-outputs if asked and
prints the line.  Its `roofline` object is the HBM roofline of the dominant kernel (the fused backward: read grad, read x,
write dx = 3 storage elements per element), from its average launch duration measured live with HIP events on the
launch stream inside the timed region.  `fwd` carries the same for the forward kernel and `step_frac` the fwd+bwd figure
BASELINE.md quotes the 70 % target on.  `traffic` = HBM bytes per backward launch from the FETCH_SIZE / WRITE_SIZE
counters, in a plain run carried from profiles/ -- `traffic_source` says so.  At N > 1 rank 0's shard step alone
(`per_gpu_efficiency`) still runs between the warm-up and the timed steps, as it always has.

`--full` adds everything else the benchmark measures or checks, each part after the timed region, on the same line:
  roofline.traffic  measured by this run: two `rocprofv3 --pmc` child passes of this same command (N = 1; `--no-measure-traffic`
                    keeps the carried figure, `--measure-traffic` asks for the passes in a plain run too)
  roofline.same_box_reference_kernels  ATen's add / copy rates on the same buffers (`--no-yardstick` skips them)
  cpu_baseline  the reference's own CPU csrc (oracle/_ref/libtorchlsq_ref_ops.so, kind "reference") -- or, if that
                build is absent, the C restatement (kind "port") -- timed on this box's host cores on the workload's
                full shape, at all cores and at 1 thread, rank 0 at N = 1 only.  A reported baseline, not the target.
                (`--no-cpu-baseline` skips it)
  secondary, roofline.sustained, config.python_ctypes_host_layer, strong_scaled  the other workloads, the headline for >= 1 s,
                the Python / ctypes host layer, BASELINE config 4 next to an N > 1 headline (`--no-secondary` skips them)
  config.collective_verified, parity_vs_reference  N > 1 and --assume-peers: the last timed step's reduced sums against the
                ranks' contributions and against the reference's per-shard digests
"""
import argparse
import glob
import json
import os
import shutil
import socket
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "lsqfakequantize-pytorch_amd"))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
METRIC = "GElem/s fake-quant fwd+bwd, per-tensor int8, 1/2/4/8 MI355X; % HBM roofline"   # BASELINE.json

# workload -> (synth config, storage dtype, channel axis override)
WORKLOADS = {
    "cfg1": ("cfg1", "float32", None),
    "cfg2": ("cfg2", "float32", None),
    "cfg3": ("cfg3", "float32", None),
    "cfg4": ("cfg4", "float32", None),
    "cfg4_shard": ("cfg4", "float32", None),           # [128,1024,14,14]: one rank's share of config 4 at 8 GPUs
    "cfg5": ("cfg5", "float32", None),
    "cfg5_bf16": ("cfg5", "bfloat16", None),
    "cfg5_axis0": ("cfg5", "float32", 0),
    # not BASELINE configs: token-layout activations (quantized axis last), the shapes the round-1 review asked about
    # not BASELINE configs either: the layouts the reference's TensorIterator walks in place (lsq_cpu.cpp:31-36,80-90) --
    #   *_misaligned      x and grad are views one element into their buffers (16-byte misaligned; outputs as the op allocates them)
    #   *_channels_last   x and grad both in channels-last memory order (per-channel on axis 1 = the memory order's LAST axis)
    #   *_mixed_layout    channels-last x, contiguous (NCHW) grad: the host layer re-orders grad first (one copy, +2 storage
    #                     elements of traffic per element)
    "cfg2_bf16": ("cfg2", "bfloat16", None),              # not a BASELINE config: config 2's per-tensor operator on bf16 storage (10 B per element)
    "cfg2_misaligned": ("cfg2", "float32", None),
    "cfg5_misaligned": ("cfg5", "float32", None), "cfg5_bf16_misaligned": ("cfg5", "bfloat16", None),
    "cfg5_channels_last": ("cfg5", "float32", None), "cfg5_mixed_layout": ("cfg5", "float32", None),
    "cfg5_bf16_channels_last": ("cfg5", "bfloat16", None), "cfg5_bf16_mixed_layout": ("cfg5", "bfloat16", None),
    "tok": ("tok", "float32", None), "tok_bf16": ("tok", "bfloat16", None),
    "vit": ("vit", "float32", None), "vit_bf16": ("vit", "bfloat16", None),
}


SECONDARY = ("cfg1", "cfg3", "cfg5", "cfg5_bf16")    # timed after the headline region of the default run
# ... as (workload, how): eager single calls first, then what the small / sharded configs look like in the forms a model runs them
SECONDARY_RUNS = tuple((w, {}) for w in SECONDARY) + (
    ("cfg4_shard", {"shard_of": 8, "note": "BASELINE config 4's per-GPU shard [128,1024,14,14]: the step ONE rank of the 8-GPU job runs "
                                           "(lsq_backward_per_tensor_wide with the global element count, fp64 sums rounded; no collective) -- "
                                           "the 1-GPU denominator of the 8-GPU efficiency target"}),
    ("cfg4_shard", {"name": "cfg4_shard_collective", "shard_of": 8, "collective": "native",
                    "note": "the SAME shard step WITH its collective, exactly as the N > 1 loop issues it (sharded_backward(..., "
                            "async_op=True), consumed one step later) in an RCCL world of ONE told it has a peer: every all-reduce "
                            "is an identity, so this is the whole per-rank call path -- extra launches, the collective's enqueue, "
                            "the stream hand-over -- without a transport between GPUs.  `collective`: native = the library's own "
                            "RCCL communicator (lsq_hip_comm_all_reduce_begin / _end), c10d = torch.distributed.all_reduce"}),
    ("cfg3", {"name": "cfg3_x50_foreach", "multi": 50,
              "note": "50 x BASELINE config 3 ([512,512,3,3] qint8 weights) per step through the multi-tensor ops "
                      "(lsq_hip_*_per_channel_multi: one launch per 32 tensors each way) -- a model's weight quantizers together"}),
    ("cfg1", {"name": "cfg1_graph", "graph": True, "note": "BASELINE config 1 replayed from a HIP graph: the GPU-side rate of a host-bound size"}),
    ("cfg3", {"name": "cfg3_graph", "graph": True, "note": "BASELINE config 3 replayed from a HIP graph"}),
)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS),
                    help="cfg2 (default; weak-scaled per GPU) | cfg4 (strong: [1024,1024,14,14] split over the ranks) | "
                         "cfg1 | cfg3, cfg5, cfg5_bf16, cfg5_axis0 (per-channel) | tok, vit (+ _bf16): [8192,4096] / [64,197,768], last axis")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run everything else the benchmark measures or checks: live PMC traffic, "
                         "ATen yardsticks, the CPU baseline, the secondary records, the collective's verification "
                         "(the --no-* options below skip parts of it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--measure-traffic", dest="measure_traffic", action="store_true", default=None,
                    help="measure roofline.traffic in this run with two rocprofv3 --pmc child passes (default in a --full run at N = 1)")
    ap.add_argument("--no-measure-traffic", dest="measure_traffic", action="store_false")
    ap.add_argument("--buffers", type=int, default=0,
                    help="input buffer sets the steps rotate through (0 = auto: as many as make the streamed working set exceed "
                         "1 GiB, so that the 256 MB Infinity Cache cannot serve the reads of a small workload; 1 = re-use one set)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full run only: skip the secondary records (cfg1, cfg3, cfg5, cfg5_bf16 timed in-process)")
    ap.add_argument("--secondary-steps", type=int, default=200, help=argparse.SUPPRESS)
    ap.add_argument("--no-yardstick", action="store_true", help="skip the ATen add / copy rates measured after the timed region")
    ap.add_argument("--host-binding", default="auto", choices=["auto", "native", "ctypes"],
                    help="host layer above the C ABI: the C++ torch binding (_lsq_torch.so) or the Python/ctypes one")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step from a HIP graph (GPU-side rate of latency-bound workloads); at N > 1 the graph holds the "
                         "sharded steps INCLUDING their all-reduces: a replay costs no per-step host time")
    ap.add_argument("--collective", default="native", choices=["native", "native-inline", "c10d"],
                    help="N > 1: the route of the one all-reduce per backward -- the library's own RCCL communicator "
                         "(lsq_hip_comm_*: `native` = on its own stream with the rounding behind it, the compute stream joined once "
                         "at the end of the region; `native-inline` = in stream order behind the backward's kernels; both fall back "
                         "to c10d when the communicator cannot be created) or torch.distributed.all_reduce")
    ap.add_argument("--backend", default="nccl", help=argparse.SUPPRESS)            # "gloo" + --single-device: smoke-test
    ap.add_argument("--single-device", action="store_true", help=argparse.SUPPRESS)  # the N>1 control flow on a 1-GPU box
    ap.add_argument("--fail-rank", type=int, default=-1, help=argparse.SUPPRESS)     # tests: this rank raises before the timed region
    ap.add_argument("--assume-peers", action="store_true",
                    help="N = 1, workload cfg4_shard: time the shard step WITH its collective over --collective, in an RCCL world of one "
                         "told it has a peer (the `cfg4_shard_collective` record of the default run as a workload of its own: for profilers)")
    ap.add_argument("--variant-fwd", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--variant-bwd", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline's LAST timed step returned (y, dx, d_scale, d_shift) as "
                         "DIR/<name>.npy in float32 (float64 storage: float64), at most 64 MB in all: larger outputs are sampled at "
                         "fixed, seeded positions (the same positions for every output of one size).  Rank 0 only at N > 1")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 without a launcher: start the ranks ourselves
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(a):
    """Start `--gpus` rank processes of this script (one per GPU) and relay rank 0's JSON line.

    Nothing here initialises the GPU: the device count comes from torch.cuda.device_count() (which does not create a
    HIP context on this image) and every rank is a fresh child process."""
    import torch
    visible = torch.cuda.device_count()
    if not a.single_device and visible < a.gpus:
        sys.stderr.write("bench.py: --gpus %d requested but only %d GPU(s) are visible; refusing to run a smaller job\n"
                         % (a.gpus, visible))
        return 2
    port = _free_port()
    procs, errs = [], []
    for r in range(a.gpus):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this pool
        env.setdefault("OMP_NUM_THREADS", "1")
        # every rank's stderr goes to its own scratch file (a pipe nobody drains would block a chatty rank): the tail of a
        # failing rank's is shown below -- a traceback on rank 5 must not vanish
        errs.append(tempfile.TemporaryFile(mode="w+", prefix="lsq_bench_rank%d_" % r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=errs[r],
                                      text=True if r == 0 else None))
    # a rank that dies early would leave the others waiting in the rendezvous: watch them all, stop the rest on a failure
    while all(p.poll() is None for p in procs):
        time.sleep(0.2)
    first_bad = [r for r, p in enumerate(procs) if p.poll() not in (None, 0)]
    if first_bad:
        time.sleep(2.0)
        for p in procs:
            if p.poll() is None:
                p.kill()                     # exactly the children started above
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out0)
    sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    for r, f in enumerate(errs):
        f.seek(0)
        text = f.read()
        f.close()
        if r in first_bad:        # the rank(s) that failed on their own, not the ones stopped because of them
            sys.stderr.write("bench.py: ---- rank %d exited with code %d; the end of its stderr ----\n%s\n" % (r, codes[r], text[-3000:]))
        elif r == 0 and not bad and text.strip():
            sys.stderr.write(text)
    if bad:
        sys.stderr.write("bench.py: rank exit codes %s\n" % bad)
        return 1
    return 0


# ---------------------------------------------------------------------------------------------------------------------
# side measurements
# ---------------------------------------------------------------------------------------------------------------------
def cpu_baseline(shape, workload):
    """Time the reference CPU path (or the port) on the workload's shape: all cores and one thread."""
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline.py"), "--shape", ",".join(str(s) for s in shape),
           "--workload", workload]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        for line in reversed(out.stdout.strip().splitlines()):
            if line.startswith("{"):
                return json.loads(line)
        return {"error": (out.stderr or out.stdout)[-400:]}
    except Exception as e:  # never let the reported baseline break the bench line
        return {"error": repr(e)}


def _pmc_mean(db_dir, counter, kernel_substr):
    dbs = sorted(glob.glob(os.path.join(db_dir, "**", "*.db"), recursive=True))
    if not dbs:
        return None
    cur = sqlite3.connect(dbs[-1]).cursor()
    q = ("select s.display_name, avg(e.value), count(*) from rocpd_pmc_event e "
         "join rocpd_info_pmc p on e.pmc_id = p.id join rocpd_kernel_dispatch d on e.event_id = d.event_id "
         "join rocpd_info_kernel_symbol s on d.kernel_id = s.id where p.name = ? group by s.display_name")
    for name, val, cnt in cur.execute(q, (counter,)):
        if kernel_substr in name:
            return float(val), int(cnt), name
    return None


def measure_traffic(a, kernel_substr):
    """HBM bytes per backward launch from the PMC counters, collected as MI355X_MICROARCH.md prescribes: separate
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes (with --kernel-trace only) over a short run of this same
    command in a child process; units KiB; gfx950 correction: FETCH_SIZE tallies the 128-byte requests of a wide
    coalesced read at 64 bytes, so it is doubled (calibrated on known-size probe kernels: profiles/r01_pmc_calibration.txt)."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None, "rocprofv3 not found"
    raw = {}
    tmp = tempfile.mkdtemp(prefix="lsq_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, ctr)
            cmd = [rocprof, "--pmc", ctr, "--kernel-trace", "-d", d, "-o", "bench", "--", sys.executable,
                   os.path.abspath(__file__), "--workload", a.workload, "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                   "--no-measure-traffic", "--no-yardstick", "--no-secondary", "--host-binding", a.host_binding]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd="/tmp", env=env)
            got = _pmc_mean(d, ctr, kernel_substr)
            if got is None:
                return None, "%s pass produced no counter rows for %s (exit %d): %s" % (ctr, kernel_substr, r.returncode,
                                                                                       (r.stderr or "")[-200:])
            raw[ctr] = got
    except Exception as e:
        return None, repr(e)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fetch_kib, write_kib = raw["FETCH_SIZE"][0], raw["WRITE_SIZE"][0]
    info = {"fetch_size_kib_raw": round(fetch_kib, 1), "write_size_kib": round(write_kib, 1),
            "dispatches_averaged": raw["FETCH_SIZE"][1], "kernel": raw["FETCH_SIZE"][2][:120],
            "formula": "(2 * FETCH_SIZE + WRITE_SIZE) * 1024"}
    return int(round((2.0 * fetch_kib + write_kib) * 1024.0)), info


DUMP_LIMIT_BYTES = 64 * 1000 * 1000     # --dump-outputs: all files together
DUMP_WHOLE_MAX = 1 << 16        # outputs of at most this many elements are written whole even when others are sampled
DUMP_SEED = 20240917


def named_outputs(y, r, reduced=None):
    """{name: tensor} of what one step hands its caller: the forward's y and the backward's (dx, d_scale, d_shift) -- or, for
    the forms that return them differently, dx and the [d_scale, d_shift] sums (`reduced`: the fp64 sums of the last
    all-reduce when the backward itself returned dx alone).  Lists (the multi-tensor ops) get an index suffix."""
    import torch
    out = {}

    def put(name, t):
        if isinstance(t, (list, tuple)):
            for i, u in enumerate(t):
                put("%s_%d" % (name, i), u)
        elif isinstance(t, torch.Tensor):
            out[name] = t

    put("y", y)
    if isinstance(r, (list, tuple)) and len(r) == 3:
        for name, t in zip(("dx", "d_scale", "d_shift"), r):
            put(name, t)
    elif isinstance(r, (list, tuple)) and len(r) == 2:
        put("dx", r[0])
        put("d_scale_d_shift", r[1])
    else:
        put("dx", r)
        if reduced is not None:
            if reduced[0] == "wide":
                put("d_scale_d_shift", reduced[1])
            else:
                put("d_scale", reduced[1])
                put("d_shift", reduced[2])
    return out


def dump_outputs(outputs, out_dir, limit=DUMP_LIMIT_BYTES):
    """Write {name: tensor} as out_dir/<name>.npy: float64 storage as float64, everything else as float32 (exact for the 16-bit
    types).  When the whole set would exceed `limit` bytes, every output of more than DUMP_WHOLE_MAX elements is reduced to the
    same share of the remaining budget, at sorted positions drawn from a fixed seed (so the samples of two outputs of one size
    -- y and dx -- sit at the same elements, and two runs sample the same elements).  Returns {name: description}."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    flat = {k: v.detach().reshape(-1) for k, v in outputs.items()}
    isz = {k: 8 if v.dtype == torch.float64 else 4 for k, v in flat.items()}
    header = 128                                                   # np.save's header, per file
    need = sum(v.numel() * isz[k] + header for k, v in flat.items())
    large = [k for k, v in flat.items() if need > limit and v.numel() > DUMP_WHOLE_MAX]
    keep = None
    if large:
        fixed = sum(flat[k].numel() * isz[k] + header for k in flat if k not in large) + header * len(large)
        keep = (limit - fixed) // sum(isz[k] for k in large)
        if keep < 1:
            raise SystemExit("--dump-outputs: %d outputs do not fit %d bytes" % (len(flat), limit))
    picks, info = {}, {}
    for k, v in flat.items():
        if k in large and v.numel() > keep:
            n = v.numel()
            if n not in picks:
                idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=keep, dtype=np.int64))
                picks[n] = (idx, torch.from_numpy(idx).to(v.device))
            v = v.index_select(0, picks[n][1])
            info[k] = {"shape": list(outputs[k].shape), "sampled": int(v.numel()), "of": n}
        else:
            v = v.view(outputs[k].shape)
            info[k] = {"shape": list(outputs[k].shape)}
        a = v.to(torch.float64 if isz[k] == 8 else torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return info


def carried_traffic(workload, n_local):
    """The committed PMC measurement of this workload (profiles/traffic_latest.json), when this run does not measure."""
    tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
    try:
        with open(tpath) as f:
            tj = json.load(f)
        entries = tj["workloads"] if "workloads" in tj else {tj.get("workload"): tj}
        e = entries.get(workload)
        if e and e.get("n_local") == n_local:
            return e.get("bwd_hbm_bytes_per_launch"), "carried from profiles/traffic_latest.json (%s); not measured in this run" % \
                e.get("source", "rocprofv3 --pmc passes of an earlier run of this command")
    except Exception:
        pass
    return None, "not measured"


# ---------------------------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------------------------
def run_rank(a):
    # multi-process GPU work on this pool needs dmabuf IPC (RCCL fails with hipIpcGetMemHandle otherwise); the
    # launcher normally exports it already
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # stdout carries ONE line, the JSON record: native libraries write there too (RCCL prints a five-line version banner
    # through C stdio whenever a communicator is created), so file descriptor 1 points at stderr until the record is printed
    sys.stdout.flush()
    stdout_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    import torchlsq  # noqa: F401
    from torchlsq import extension, synth
    from torchlsq.distributed import sharded_backward

    extension._assert_has_ops()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if not a.single_device and torch.cuda.device_count() <= local_rank:
        raise SystemExit("rank %d: no GPU %d on this node (%d visible)" % (rank, local_rank, torch.cuda.device_count()))
    dev = torch.device("cuda", 0 if a.single_device else local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)   # "nccl" == RCCL on ROCm
        else:
            dist.init_process_group(backend=a.backend)

    if a.fail_rank == rank:
        raise RuntimeError("deliberate failure of rank %d (--fail-rank)" % rank)
    if a.variant_fwd or a.variant_bwd:      # launch variants: tools build of the library (tools/lsq_tools.py), ctypes host layer
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import lsq_tools
        lsq_tools.activate()
        a.host_binding = "ctypes"
    if a.host_binding == "native":
        extension.set_host_binding("native")
    elif a.host_binding == "ctypes":
        extension.set_host_binding("ctypes")
    binding = extension.host_binding()
    # the ops of the hot path on the chosen host layer: torch.ops.torchlsq_native.* (C++ binding) or torch.ops.torchlsq.*
    # (Python torch.library registration over ctypes); both end in the same C-ABI call
    ops = torch.ops.torchlsq_native if binding == "native" else torch.ops.torchlsq
    ops_of = {"native": getattr(torch.ops, "torchlsq_native", None), "ctypes": torch.ops.torchlsq}

    one = {"up": False}
    route_info = [None]        # lsq_hip_comm_info of the library's communicator, once one exists (which side stream was picked)

    def ensure_world_of_one():
        """an RCCL process group of ONE rank for the single-GPU `*_collective` records (every all-reduce an identity)"""
        if one["up"] or dist.is_initialized():
            return
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(_free_port())
        dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
        one["up"] = True

    preflight = {}

    def native_preflight():
        """N > 1 (or --assume-peers), native routes: BEFORE anything is timed the library's communicator is created and CHECKED
        (torchlsq.distributed.native_comm: every rank agrees at every step of the creation; the ranks add up rank + 1 under a
        host-side deadline; then the very route that will be timed -- begin on the communicator's stream, a consumer behind it
        there, one join -- carries 128 reductions of changing values, first with events that skip the system-scope fence, with
        fenced events if any rank saw a wrong value), and this run repeats the route check on the stream its steps run on.  If
        anything fails -- no communicator, a wrong sum, a reduction that never finishes -- every rank takes torch.distributed's
        route for the whole run and the record says so: the first time this communicator meets real peers is a driver run nobody
        can repeat, and a hang there would cost the whole scaling record.  (A reduction that hung stays on its own stream; the
        process then leaves through os._exit once the line is out.)"""
        from torchlsq import distributed as D
        t0 = time.perf_counter()
        ok, why, comm = 1, "", None
        D.set_native_collective(True)
        try:
            if a.assume_peers:
                ensure_world_of_one()
                D.assume_peers(True)
            comm = D.native_comm(None, dev)          # collective: the id over torch.distributed, every verdict MIN-reduced
        except Exception as e:
            why = "communicator: %r" % (e,)
        finally:
            if a.assume_peers:
                D.assume_peers(False)
        hung = False
        if comm is None:
            ok, why = 0, why or D.LAST_FAILURE.get("why") or "no native communicator (RCCL not resolvable, or a rank could not join)"
            hung = bool(D.LAST_FAILURE.get("hung"))
        else:
            limit = float(os.environ.get("LSQ_BENCH_PREFLIGHT_S", "30"))      # (tests: a negative limit = "it never finished")
            try:
                bad = D.check_timed_route(comm, dev, limit)      # the timed route, on the stream the steps will run on
            except Exception as e:
                bad = "route check: %r" % (e,)
            if bad == "hung":
                ok, why, hung = 0, "a reduction of 24 bytes on the timed route did not finish in time", True
            elif bad:
                ok, why = 0, bad
        if os.environ.get("LSQ_BENCH_PREFLIGHT_FAIL") == "1":        # (tests: the fall-back path without a broken transport)
            ok, why = 0, why or "LSQ_BENCH_PREFLIGHT_FAIL=1"
        flag = torch.tensor([ok, -int(hung)], dtype=torch.int32, device=dev)
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)              # torch.distributed's own communicator and stream
        agreed, hung = int(flag[0].item()), bool(int(flag[1].item()) < 0)      # (hung anywhere: nobody tears that communicator down)
        preflight.update(route="native" if agreed else "c10d", ok=bool(agreed), seconds=round(time.perf_counter() - t0, 3),
                         checked="sum of rank + 1 over %d rank(s) in stream order, then %d reductions of changing values through the "
                                 "TIMED route (begin on the communicator's stream, consumer behind it, join), at creation and again on "
                                 "the stream the steps run on" % (comm.nranks if comm is not None else world, D.ROUTE_CHECK_REDUCTIONS))
        if comm is not None and comm.checked:
            preflight["events"] = comm.checked.get("events")
        if not agreed:
            preflight["why"] = why or "another rank failed"
            preflight["hung"] = hung
            a.collective = "c10d"
            D.set_native_collective(False)
            if hung:
                D._COMMS.clear()            # never destroyed: its stream holds a reduction that will not end
            else:
                try:
                    D.destroy_native_comms()
                except Exception:
                    D._COMMS.clear()
        return agreed

    _shard_digests = {}

    def shard_digests():
        """tests/golden/shard_digests.json (made by tests/golden/make_golden.py --shards from the reference's CPU ops): what every
        rank of a batch-sharded run of config 4 / weak-scaled config 2 must hold"""
        if not _shard_digests:
            try:
                with open(os.path.join(ROOT, "tests", "golden", "shard_digests.json")) as f:
                    _shard_digests.update(json.load(f)["shards"])
            except Exception as e:
                _shard_digests["error"] = repr(e)
        return _shard_digests

    def verify_sharded(reduced, workload, c, dt, shape, x0, g0, scale, shift, per_channel, axis, tail, n_scaler, ops, fwd_of, shard_of, route):
        """What the timed region's LAST step reduced, proven twice (every rank runs this; the verdicts are MIN-agreed):

        collective_verified -- the reduced [sum ds, sum db] against the ranks' own contributions, recomputed here with the same
          kernel (lsq_backward_*_wide, the global element count in the scaler: bit-reproducible) and carried by an independent
          transport: torch.distributed's all_gather, added up in rank order in fp64.  The two differ only in the ORDER the N
          doubles were added: |reduced - gathered| <= 1e-12 * sum_r |contribution_r| (a rounded fp32 result of the in-order route:
          + one fp32 rounding).  The ranks hold different data (their own slices), so a stale, dropped or doubled contribution
          cannot cancel out.
        parity_vs_reference -- where tests/golden/shard_digests.json has the workload (BASELINE config 4 at 2 / 4 / 8 ranks and
          its 1/8 shard; weak-scaled config 2 at 2 / 4 / 8): each rank's y and dx by sha256 against the reference CPU csrc's
          outputs for its slice (bit-exact), each rank's contribution and the reduced sums against the reference's d_scale /
          d_shift on the concatenated tensor, |got - ref| <= 1e-6 * sum|terms| (north_star's bar; the contract is
          lsq_cpu.cpp:103-104,138-139 on the whole batch)."""
        import hashlib
        C = scale.numel() if per_channel else 1
        if reduced[0] == "wide":
            red = reduced[1].detach().to(torch.float64).reshape(2, -1).clone()
            rounded = False
        else:
            red = torch.stack([reduced[1].detach().reshape(-1), reduced[2].detach().reshape(-1)]).to(torch.float64)
            rounded = True
        if os.environ.get("LSQ_BENCH_CORRUPT_REDUCED") == "1":          # (tests: a wrong sum must show as ok: false, and still print)
            red = red * (1.0 + 1e-3)
        if per_channel:
            dx_l, wide_l = ops.lsq_backward_per_channel_wide(g0, x0, scale, shift, axis, *tail, n_scaler)
            y_l = fwd_of(x0, scale, shift, axis, *tail)
        else:
            dx_l, wide_l = ops.lsq_backward_per_tensor_wide(g0, x0, scale, shift, *tail, n_scaler)
            y_l = fwd_of(x0, scale, shift, *tail)
        mine = wide_l.detach().to(torch.float64).reshape(2, -1)
        real_world = dist.get_world_size() if dist.is_initialized() else 1
        if real_world > 1:
            parts = [torch.zeros_like(mine) for _ in range(real_world)]
            dist.all_gather(parts, mine.contiguous())
        else:
            parts = [mine]
        total = torch.zeros_like(mine)
        mag = torch.zeros_like(mine)
        for p_ in parts:                       # rank order, fp64
            total = total + p_
            mag = mag + p_.abs()
        tol = 1e-12 * mag + (1.2e-7 * total.abs() if rounded else 0.0) + 1e-300
        err = (red - total).abs()
        ok_col = bool((err <= tol).all().item())
        worst = int(torch.argmax(err / tol).item())
        col = {"ok": ok_col, "route": route, "ranks": real_world, "what": "the last timed step's reduced [sum ds, sum db] vs the ranks' own "
               "contributions (recomputed, bit-reproducible kernel) all-gathered over torch.distributed and added in rank order",
               "tolerance": "1e-12 * sum_r |contribution_r|" + (" + 1 fp32 rounding (the in-order route returns rounded sums)" if rounded else ""),
               "max_err_over_tol": float((err / tol).max().item()),
               "reduced": [float(red[0].reshape(-1)[worst % red.shape[1]].item()), float(red[1].reshape(-1)[worst % red.shape[1]].item())],
               "gathered": [float(total[0].reshape(-1)[worst % red.shape[1]].item()), float(total[1].reshape(-1)[worst % red.shape[1]].item())],
               "slots": int(red.numel()), "distinct_data_per_rank": real_world > 1}
        # ---- against the reference's outputs for this rank's slice
        par = {"ok": None, "why": "no reference digests for this workload / world size (tests/golden/shard_digests.json holds BASELINE config 4 "
                                  "at 2, 4, 8 ranks and weak-scaled config 2 at 2, 4, 8)"}
        sd = shard_digests()
        key, nw = None, shard_of
        if dt == torch.float32 and "error" not in sd:
            if workload in ("cfg4", "cfg4_shard") and str(nw) in sd.get("cfg4", {}).get("by_world", {}):
                key = "cfg4"
            elif workload == "cfg2" and str(nw) in sd.get("cfg2_weak", {}).get("by_world", {}):
                key = "cfg2_weak"
        if key is not None:
            bw = sd[key]["by_world"][str(nw)]
            exp = bw["shards"][rank]
            exp_sha = exp if key == "cfg4" else sd[key]["shards"][rank]
            ysha = hashlib.sha256(memoryview(y_l.detach().cpu().contiguous().numpy()).cast("B")).hexdigest()
            dxsha = hashlib.sha256(memoryview(dx_l.detach().cpu().contiguous().numpy()).cast("B")).hexdigest()
            sha_ok = ysha == exp_sha["y_sha256"] and dxsha == exp_sha["dx_sha256"]
            m_ds, m_db = float(mine[0, 0].item()), float(mine[1, 0].item())
            mine_ok = abs(m_ds - exp["ds_wide"]) <= 1e-6 * exp["abs_ds"] and abs(m_db - exp["db_wide"]) <= 1e-6 * exp["abs_db"]
            if key == "cfg4":
                ref_ds, ref_db = sd[key]["ds"][0], sd[key]["db"][0]
                ref_is = "the reference CPU csrc's d_scale / d_shift on the whole [1024,1024,14,14] tensor"
            else:
                ref_ds, ref_db = bw["sum_ds_wide"], bw["sum_db_wide"]
                ref_is = "the sum of the ranks' contributions from the pinned oracle run with the global count (the reference's terms)"
            if real_world == nw:
                red_ok = abs(float(red[0, 0].item()) - ref_ds) <= 1e-6 * bw["abs_ds"] and abs(float(red[1, 0].item()) - ref_db) <= 1e-6 * bw["abs_db"]
                red_note = {"reduced": [float(red[0, 0].item()), float(red[1, 0].item())], "reference": [ref_ds, ref_db],
                            "budget_1e-6_sum_abs_terms": [1e-6 * bw["abs_ds"], 1e-6 * bw["abs_db"]], "reference_is": ref_is}
            else:           # a world of one told it has peers: the "sum" is this rank's own contribution
                red_ok, red_note = True, {"reduced": "n/a: %d real rank(s) of %d -- only this rank's contribution is checked" % (real_world, nw)}
            flags = torch.tensor([int(sha_ok), int(mine_ok), int(red_ok)], dtype=torch.int32, device=dev)
            if real_world > 1:
                dist.all_reduce(flags, op=dist.ReduceOp.MIN)
            f = [bool(v) for v in flags.tolist()]
            par = {"ok": all(f), "digests": "tests/golden/shard_digests.json[%s][by_world][%d]" % (key, nw),
                   "y_dx_sha256_all_ranks_match_reference_slices": f[0], "each_rank_contribution_within_1e-6_sum_abs_terms": f[1],
                   "reduced_within_1e-6_sum_abs_terms": f[2], "ranks_checked": real_world}
            par.update(red_note)
            if rank == 0 and not f[0]:
                par["rank0_sha"] = {"y": ysha, "dx": dxsha, "expected_y": exp_sha["y_sha256"], "expected_dx": exp_sha["dx_sha256"]}
        flag = torch.tensor([int(ok_col)], dtype=torch.int32, device=dev)
        if real_world > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        col["ok"] = bool(int(flag.item()))
        del y_l, dx_l
        return {"collective_verified": col, "parity_vs_reference": par}

    def measure(workload, steps, warmup, graph=False, buffers=0, ops=ops, warm_ms=0.0, extra_blocks=0, shard_of=0, multi=0,
                collective=None, inputs=None, shape_override=None, event_every=0, keep_outputs=False):
        """Time `steps` steps (forward op + backward op) of one workload after `warmup` untimed ones; returns the raw
        measurements (K-step wall time bracketed by barrier + synchronize, max over ranks; per-op HIP-event times).
        shard_of = R (single rank only): the step ONE rank of an R-rank job runs on this shape -- the `*_wide` backward with
        the global element count (R x local) in the gradient scaler and the rounding of the fp64 sums, no collective.
        multi = M (per-channel weights): M tensors of the shape per step through the multi-tensor ops (one launch per 32).
        collective = "native" | "c10d" (single rank, with shard_of): the N > 1 step itself -- sharded_backward(async_op=True) and
        its drain -- with the process group told it has peers (torchlsq.distributed.assume_peers), over the named route.
        inputs = (xs, gs, scale, shift) of an earlier measure() of the same workload: run on those very buffers.
        shape_override: another shape for the same workload's operator (the host-cost probe on a tiny tensor).
        keep_outputs: return what the last timed step handed back (`outputs`, see named_outputs) for --dump-outputs."""
        cfg_name, dtype_name, axis_override = WORKLOADS[workload]
        c = dict(synth.CONFIGS[cfg_name])
        if axis_override is not None:
            c["axis"] = axis_override
        dt = getattr(torch, dtype_name)
        esz = 2 if dt in (torch.bfloat16, torch.float16) else 4
        per_channel = c["per_channel"]
        shape = list(c["shape"])
        scaling = "weak"
        if workload == "cfg4":           # strong scaling: fixed global batch split over the ranks
            assert shape[0] % world == 0
            shape[0] //= world
            scaling = "strong"
        if workload == "cfg4_shard":     # one rank's share of config 4 at 8 GPUs, whatever this job's size
            shape[0] //= 8
            if world == 1 and not shard_of:
                shard_of = 8             # ... run as that rank runs it: global element count in the scaler, fp64 sums rounded
        if world > 1 and per_channel and c["axis"] == 0:
            raise SystemExit("workload %s quantises along dim 0, the sharded dim: a weight is replicated under data "
                             "parallelism, there is nothing to shard -- run it with --gpus 1" % workload)
        if shape_override is not None:
            shape = list(shape_override)
        if inputs is not None:
            xs_in, gs_in, scale, shift = inputs
            x, g = xs_in[0], gs_in[0]
        else:
            # N > 1: rank r holds ITS slice of the batch -- rows [r * rows, (r + 1) * rows) of the global tensor (config 4: of
            # [1024,1024,14,14]; the weak-scaled workloads: of a virtual tensor N times the per-GPU shape), the same bits that
            # slice of the whole tensor has (synth.make_inputs(first_index)); the ranks do NOT hold copies of one shard
            n_shard = 1
            for d_ in shape:
                n_shard *= d_
            x, g, scale, shift = synth.make_inputs(c, device=dev, dtype=dt, shape=shape, first_index=rank * n_shard if world > 1 else 0)
        # the layout variants (WORKLOADS): every buffer set gets the same treatment
        def relayout(t, is_grad):
            if workload.endswith("_misaligned"):
                home = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
                v = home[1:1 + t.numel()].view(t.shape)
                v.copy_(t)
                assert v.data_ptr() % 16 != 0
                return v
            if workload.endswith("_channels_last") or (workload.endswith("_mixed_layout") and not is_grad):
                return t.contiguous(memory_format=torch.channels_last)
            return t.clone()
        if inputs is None and workload.rsplit("_", 1)[-1] in ("misaligned", "last", "layout"):
            x, g = relayout(x, False), relayout(g, True)
        else:
            relayout = None
        n_local = x.numel()
        # Small workloads re-using one set of buffers are partly served by the 256 MB Infinity Cache (config 5 streams 308 MB per
        # step in fp32, 154 MB in bf16), which is not the HBM rate the roofline is about: the steps rotate through `n_sets`
        # copies of (x, grad), more than 1 GiB of inputs in total.  Config 2 (2.4 GB per step) needs one set.
        set_bytes = 2 * n_local * esz
        n_sets = buffers if buffers > 0 else max(1, min(16, -(-(1 << 30) // set_bytes)))
        if multi:
            assert per_channel and world == 1 and not shard_of
            set_bytes *= multi
            n_sets = buffers if buffers > 0 else max(1, min(16, -(-(1 << 30) // set_bytes)))
            xs = [[x] + [x.clone() for _ in range(multi - 1)] for _ in range(n_sets)]
            gs = [[g] + [g.clone() for _ in range(multi - 1)] for _ in range(n_sets)]
            scales, shifts, axes = [scale.clone() for _ in range(multi)], [shift.clone() for _ in range(multi)], [c["axis"]] * multi
            n_local *= multi
        elif inputs is not None:
            xs, gs = list(xs_in), list(gs_in)
            n_sets = len(xs)
        else:
            xs, gs = [x], [g]
            for _ in range(n_sets - 1):
                xs.append(relayout(x, False) if relayout else x.clone())
                gs.append(relayout(g, True) if relayout else g.clone())
        cur = [0]

        def bset():       # the backward works on a set the forward touched n_sets / 2 steps ago: not on lines the forward just read
            return (cur[0] + n_sets // 2) % n_sets
        n_global = n_local * world
        n_scaler = n_local * shard_of if shard_of else 0
        if collective:
            assert world == 1 and shard_of and not multi
            ensure_world_of_one()
        q = (c["qmin"], c["qmax"], c["tmin"], c["tmax"])
        sym = not c["affine"]
        axis = c["axis"]
        tail = q + (True, 1.0, sym, False, False)
        # the ops' `default` overloads, looked up once (what functional.lsq and the modules hold on to as well): a call
        # through the overload packet re-resolves the overload every time, ~1 us of host time per op
        op_fwd_pc, op_fwd_pt = ops.lsq_forward_per_channel.default, ops.lsq_forward_per_tensor.default
        op_bwd_pc, op_bwd_pt = ops.lsq_backward_per_channel.default, ops.lsq_backward_per_tensor.default

        native_multi = multi and ops is getattr(torch.ops, "torchlsq_native", None)

        def fwd():
            if multi:
                if native_multi:
                    return ops.lsq_forward_per_channel_multi(xs[cur[0]], scales, shifts, axes, *tail)
                return extension.hip_forward_per_channel_multi(xs[cur[0]], scales, shifts, axes, *tail)
            if a.variant_fwd:
                if per_channel:
                    return extension.hip_forward_per_channel(xs[cur[0]], scale, shift, axis, *tail, variant=a.variant_fwd)
                return extension.hip_forward_per_tensor(xs[cur[0]], scale, shift, *tail, variant=a.variant_fwd)
            if per_channel:
                return op_fwd_pc(xs[cur[0]], scale, shift, axis, *tail)
            return op_fwd_pt(xs[cur[0]], scale, shift, *tail)

        pending = []   # N > 1: the previous step's in-flight all-reduce (RCCL runs it on its own stream)
        last_reduced = [None]   # what the LAST sharded backward's collective produced: ("wide", fp64 [2, C]) or ("rounded", ds, db)

        def bwd():
            if multi:
                if native_multi:
                    return ops.lsq_backward_per_channel_multi(gs[bset()], xs[bset()], scales, shifts, axes, *tail)
                return extension.hip_backward_per_channel_multi(gs[bset()], xs[bset()], scales, shifts, axes, *tail)
            if collective:      # ... and WITH it: the N > 1 branch below, in a world of one told it has peers
                if collective == "native-inline":       # the reduction in stream order, right behind the backward's kernels
                    r3 = sharded_backward(gs[bset()], xs[bset()], scale, shift, *q, axis, True, 1.0, c["affine"], per_channel, False, False,
                                          None, n_scaler)
                    last_reduced[0] = ("rounded", r3[1], r3[2])
                    return r3
                dx, wide, work = sharded_backward(gs[bset()], xs[bset()], scale, shift, *q, axis, True, 1.0, c["affine"], per_channel, False, False,
                                                  None, n_scaler, async_op=True)
                drain()
                pending.append((wide, work))
                last_reduced[0] = ("wide", wide)
                return dx
            if shard_of:        # one rank's step of a shard_of-rank job: everything but the collective itself
                if per_channel:
                    dx, wide = ops.lsq_backward_per_channel_wide(gs[bset()], xs[bset()], scale, shift, axis, *tail, n_scaler)
                else:
                    dx, wide = ops.lsq_backward_per_tensor_wide(gs[bset()], xs[bset()], scale, shift, *tail, n_scaler)
                return dx, wide.to(torch.float32)
            if world == 1:
                if a.variant_bwd:
                    if per_channel:
                        return extension.hip_backward_per_channel(gs[bset()], xs[bset()], scale, shift, axis, *tail, variant=a.variant_bwd)
                    return extension.hip_backward_per_tensor(gs[bset()], xs[bset()], scale, shift, *tail, variant=a.variant_bwd)
                if per_channel:
                    return op_bwd_pc(gs[bset()], xs[bset()], scale, shift, axis, *tail)
                return op_bwd_pt(gs[bset()], xs[bset()], scale, shift, *tail)
            # batch-sharded: local fused backward with the GLOBAL numel in the gradient scaler, then ONE
            # all-reduce of the packed fp64 [d_scale, d_shift] sums.  The collective is issued async and
            # consumed one step later (d_scale/d_shift are only needed by the optimizer), so its latency
            # hides behind the next step's kernels; every reduction is completed inside the timed region.
            if a.collective == "native-inline":
                r3 = sharded_backward(gs[bset()], xs[bset()], scale, shift, *q, axis, True, 1.0, c["affine"], per_channel, False, False,
                                      None, n_global)
                last_reduced[0] = ("rounded", r3[1], r3[2])
                return r3
            dx, wide, work = sharded_backward(gs[bset()], xs[bset()], scale, shift, *q, axis, True, 1.0, c["affine"], per_channel, False, False,
                                              None, n_global, async_op=True)
            drain()
            pending.append((wide, work))
            last_reduced[0] = ("wide", wide)
            return dx

        last_native = [None]

        def drain(final=False):
            # torch.distributed route: the stream waits for the previous step's reduction, then rounds it.  Native route: the
            # reduction AND the rounding run on the communicator's stream (work.rounded), the compute stream is joined ONCE,
            # at the end of the region (final) -- what a training step does before its optimizer reads the gradients
            while pending:
                wide, work = pending.pop()
                if getattr(work, "deferred", False):
                    last_native[0] = work
                    continue
                work.wait()                                   # stream-level wait, the host does not block
                ds_db = wide.to(torch.float32)                # the rounding to the parameter type
            if final and last_native[0] is not None:
                last_native[0].wait()                         # joins every earlier reduction too: the side stream is in order
                last_native[0] = None
            return None

        if collective or world > 1:
            from torchlsq import distributed as D
            D.set_native_collective((collective or a.collective).startswith("native"))
            if collective:
                D.assume_peers(True)
        step_graphs = None
        graph_steps = 1
        if graph:
            # ONE graph holding `graph_steps` consecutive steps (the buffer sets in rotation): a replay is one launch of the
            # whole chain, so what is timed is the GPU-side rate -- a graph per step would still pay a graph launch (~10 us of
            # host time on this stack) per 10 us step.  The step count is rounded up to whole replays.
            graph_steps = n_sets if (n_sets >= 8 or set_bytes >= (64 << 20)) else 8
            steps = -(-steps // graph_steps) * graph_steps
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for k in range(n_sets):
                    cur[0] = k
                    fwd(); bwd()
                drain(final=True)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=st):
                    for k in range(graph_steps):
                        cur[0] = k % n_sets
                        y = fwd()
                        r = bwd()
                    drain(final=True)   # every collective begun inside the capture is joined inside it (the side stream rejoins)
                step_graphs = [gr]
            torch.cuda.synchronize()

        # `warmup` untimed steps -- and, for the secondary records, as many more as it takes to fill `warm_ms` of wall time:
        # they are timed after this process has sat through the CPU baseline (GPU idle for 20 s), and twenty steps of a
        # 20 us workload do not bring the clocks back
        t_warm = time.perf_counter()
        i = 0
        while i < warmup or (warm_ms > 0 and world == 1 and (time.perf_counter() - t_warm) * 1e3 < warm_ms):
            cur[0] = i % n_sets
            if step_graphs is not None:
                step_graphs[0].replay()
                i += graph_steps - 1
            else:
                y = fwd()
                r = bwd()
            i += 1
            if warm_ms > 0 and i % 64 == 0:
                torch.cuda.synchronize()
        drain(final=True)
        torch.cuda.synchronize()

        # N > 1: rank 0's shard step ALONE (same kernels, the global element count in the scaler, no collective) while the
        # other ranks wait at a barrier -- the numerator of `per_gpu_efficiency`
        solo_ms = None
        if world > 1:
            def bwd_local():
                if per_channel:
                    return ops.lsq_backward_per_channel_wide(gs[bset()], xs[bset()], scale, shift, axis, *tail, n_global)
                return ops.lsq_backward_per_tensor_wide(gs[bset()], xs[bset()], scale, shift, *tail, n_global)
            dist.barrier()
            torch.cuda.synchronize()
            if rank == 0:
                ts = time.perf_counter()
                for i in range(steps):
                    cur[0] = i % n_sets
                    y = fwd()
                    r = bwd_local()
                torch.cuda.synchronize()
                solo_ms = (time.perf_counter() - ts) / steps * 1e3
            dist.barrier()
            torch.cuda.synchronize()

        # HIP events bracket the forward and the backward op on every `stride`-th step of the timed region: ten to nineteen
        # sampled steps.  (An event record is 2-3 us of host time and drains the queue: bracketing every op of every step
        # would cost a few % of a 0.7 ms step, and three records on every fourth step -- the earlier rule -- still cost the
        # host-bound 20 us workloads about a tenth of their step.  Under --graph the ops are nodes of one graph launch, so
        # the per-op split comes from a second, un-timed pass of eager launches.)
        stride = event_every if event_every > 0 else max(1, steps // 10)     # (event_every: the sustained record samples 1 % of its steps)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] if i % stride == 0 else None for i in range(steps)]
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if step_graphs is not None:
            for i in range(steps // graph_steps):
                step_graphs[0].replay()
        else:
            for i in range(steps):
                cur[0] = i % n_sets
                e = ev[i]
                if e is None:
                    y = fwd()
                    r = bwd()
                else:
                    e[0].record()
                    y = fwd()
                    e[1].record()
                    r = bwd()
                    e[2].record()
        drain(final=True)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        last = (y, r) if keep_outputs else None        # the last timed step's outputs (a graph's: its last step, as replayed)
        if step_graphs is not None:
            for i, e in enumerate(ev):
                if e is not None:
                    cur[0] = i % n_sets
                    e[0].record(); y = fwd(); e[1].record(); r = bwd(); e[2].record()
            torch.cuda.synchronize()

        # secondary records (single rank, eager): `extra_blocks` more blocks of the same K steps without events; the record
        # takes the MEDIAN block -- one 5 ms hiccup of the box (seen: a 200-step block of config 5 bf16 at 18 ms instead of
        # 10.7) would otherwise halve a number that is only reported once
        block_times = [elapsed]
        if extra_blocks > 0 and world == 1 and step_graphs is None:
            for _ in range(extra_blocks):
                torch.cuda.synchronize()
                tb = time.perf_counter()
                for i in range(steps):
                    cur[0] = i % n_sets
                    y = fwd()
                    r = bwd()
                drain(final=True)
                torch.cuda.synchronize()
                block_times.append(time.perf_counter() - tb)
            elapsed = sorted(block_times)[len(block_times) // 2]
            if keep_outputs:
                last = (y, r)

        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_max = float(t.item())

        fwd_ms = sorted(e[0].elapsed_time(e[1]) for e in ev if e is not None)
        bwd_ms = sorted(e[1].elapsed_time(e[2]) for e in ev if e is not None)
        fwd_avg = sum(fwd_ms) / len(fwd_ms)
        bwd_avg = sum(bwd_ms) / len(bwd_ms)
        route = None
        if collective or world > 1:
            from torchlsq import distributed as D
            comm = D.native_comm(None, dev, create=False)
            route = "native" if comm is not None else "c10d"
            if comm is not None:
                try:
                    route_info[0] = comm.info()
                except Exception:
                    pass
            if collective:
                D.assume_peers(False)
            D.set_native_collective(a.collective.startswith("native"))

        verified = None
        if a.full and (collective or world > 1) and last_reduced[0] is not None:
            try:
                verified = verify_sharded(last_reduced[0], workload, c, dt, shape, xs[0], gs[0], scale, shift, per_channel, axis, tail,
                                          n_scaler if collective else n_global, ops, fwd_of=(op_fwd_pc if per_channel else op_fwd_pt),
                                          shard_of=shard_of if collective else world, route=route)
            except Exception as e:      # every rank takes the same path; the line must come out either way
                import traceback
                traceback.print_exc()
                verified = {"collective_verified": {"ok": False, "error": repr(e)}, "parity_vs_reference": {"ok": False, "error": repr(e)}}

        return dict(workload=workload, c=c, dtype_name=dtype_name, esz=esz, per_channel=per_channel, shape=shape, axis=axis, verified=verified,
                    scaling=scaling, n_local=n_local, n_global=n_global, n_sets=n_sets, set_bytes=set_bytes, steps=steps,
                    warmup=warmup, elapsed_max=elapsed_max, fwd_ms=fwd_ms, bwd_ms=bwd_ms, fwd_avg=fwd_avg, bwd_avg=bwd_avg,
                    xs=xs, gs=gs, x=x, scale=scale, shift=shift, solo_ms=solo_ms, block_times=block_times, graph=bool(graph),
                    graph_steps=graph_steps, collective_route=route,
                    outputs=named_outputs(last[0], last[1], last_reduced[0]) if last is not None else None)

    # the non-headline workloads are small (20-100 us per step): W warm-up steps are over before the GPU's clocks have come up,
    # so they warm up for at least 60 ms of wall time (the headline workload, cfg2, does exactly its W steps)
    warm_floor_ms = 0.0 if (a.workload == "cfg2" or world > 1) else 60.0      # (N > 1: every rank must run the same steps)
    # ... and they report the median of three blocks of K steps (the headline: exactly its K steps, once)
    extra_blocks = 0 if (a.workload == "cfg2" or world > 1 or a.graph) else 2
    head_kw = {}
    if a.assume_peers:
        if world != 1 or a.workload != "cfg4_shard":
            raise SystemExit("--assume-peers is for --gpus 1 --workload cfg4_shard")
        head_kw = dict(shard_of=8, collective=a.collective)
    if (world > 1 and a.backend == "nccl" or a.assume_peers) and a.collective.startswith("native"):
        native_preflight()
        if a.assume_peers:
            head_kw["collective"] = a.collective
    m = measure(a.workload, a.steps, a.warmup, a.graph, a.buffers, warm_ms=warm_floor_ms, extra_blocks=extra_blocks,
                keep_outputs=bool(a.dump_outputs), **head_kw)
    dumped = None
    if a.dump_outputs and rank == 0:
        dumped = dump_outputs(m["outputs"], a.dump_outputs)
    m["outputs"] = None
    c, dtype_name, esz, per_channel, shape, axis = m["c"], m["dtype_name"], m["esz"], m["per_channel"], m["shape"], m["axis"]
    scaling, n_local, n_global, n_sets, set_bytes = m["scaling"], m["n_local"], m["n_global"], m["n_sets"], m["set_bytes"]
    elapsed_max, fwd_ms, bwd_ms, fwd_avg, bwd_avg = m["elapsed_max"], m["fwd_ms"], m["bwd_ms"], m["fwd_avg"], m["bwd_avg"]
    xs, gs, x = m["xs"], m["gs"], m["x"]
    if rank == 0:
        bytes_fwd, bytes_bwd = 2 * esz, 3 * esz   # algorithmic bytes per element: R x + W y; R grad + R x + W dx
        value = n_global * m["steps"] / elapsed_max / 1e9
        bwd_gbs = bytes_bwd * n_local / (bwd_avg * 1e-3) / 1e9
        fwd_gbs = bytes_fwd * n_local / (fwd_avg * 1e-3) / 1e9
        step_gbs = (bytes_fwd + bytes_bwd) * n_local / ((fwd_avg + bwd_avg) * 1e-3) / 1e9
        io = {"float32": "io_f32", "bfloat16": "io_bf16"}[dtype_name]
        if per_channel:
            outer = 1
            for d_ in shape[:axis]:
                outer *= d_
            inner = 1
            for d_ in shape[axis + 1:]:
                inner *= d_
            seg = outer < 8 and inner % (16 // esz) == 0 and inner >= 256 * (16 // esz)    # lsq_pc_geom.hpp pick_segment_mode
            kb, kf = ("bwd_seg_kernel", "fwd_seg_kernel") if seg else ("bwd_pc_kernel", "fwd_pc_kernel")
            what = "per-channel %s (qmin,qmax=%d,%d; axis %d: [outer,C,inner]=[%d,%d,%d], %s mode)" % (
                "qint8" if c["qmin"] < 0 else "quint8", c["qmin"], c["qmax"], axis, outer, shape[axis], inner,
                "segment" if seg else "window")
            opnames = "lsq_forward_per_channel + lsq_backward_per_channel"
        else:
            kb, kf = "bwd_pt_kernel", "fwd_pt_kernel"
            what = "per-tensor quint8 (qmin,qmax=%d,%d)" % (c["qmin"], c["qmax"])
            opnames = "lsq_forward_per_tensor + lsq_backward_per_tensor"
        traffic, traffic_source = None, "not measured"
        # --full: measure at N = 1 -- unless this process itself runs under a profiler (a nested rocprofv3 is asking for trouble)
        profiled = any("rocprof" in os.environ.get(k, "").lower() for k in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB"))
        want_pmc = a.measure_traffic if a.measure_traffic is not None else (a.full and world == 1 and not a.graph and not profiled)
        if want_pmc and world == 1:
            traffic, info = measure_traffic(a, "lsq::" + kb)
            if traffic is not None:
                traffic_source = dict(info, how="measured by this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE child "
                                                "passes (separate, --kernel-trace only) over 3 steps of this same command")
            else:
                carried, src = carried_traffic(a.workload, n_local)
                traffic, traffic_source = carried, "live PMC passes failed (%s); %s" % (info, src)
        else:
            traffic, traffic_source = carried_traffic(a.workload, n_local)
        metric = METRIC if not per_channel else METRIC.replace("per-tensor int8", "per-channel (%s workload, not the BASELINE headline)" % a.workload)
        line = {
            "metric": metric,
            "value": round(value, 3), "unit": "GElem/s", "n_gpus": world, "steps": m["steps"], "warmup": a.warmup,
            "ms_per_step": round(elapsed_max / m["steps"] * 1e3, 5), "higher_is_better": True, "scaling": scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "run": "full" if a.full else "plain",
            "warmup_wall_floor_ms": warm_floor_ms,
            "timed_blocks_ms_per_step": [round(tb / m["steps"] * 1e3, 5) for tb in m["block_times"]],
            "config": {"workload": "%s: %s %s %s per GPU, %s%s" % (a.workload, what, dtype_name, shape, opnames,
                                                                    "" if world == 1 else ", batch-sharded, 1 RCCL all-reduce of fp64 [ds,db] per step"),
                       "storage": dtype_name, "arithmetic": "float32",
                       "layout": ("x and grad one element into their buffers (16-byte misaligned views)" if a.workload.endswith("_misaligned") else
                                  "x and grad in channels-last memory order: the kernels see [N*H*W, C, 1]" if a.workload.endswith("_channels_last") else
                                  "channels-last x, contiguous grad: the host layer re-orders grad into x's memory order first (a copy)"
                                  if a.workload.endswith("_mixed_layout") else "contiguous"),
                       "elements_per_gpu": n_local, "global_elements": n_global,
                       "parallelism": "dp%d" % world, "host_binding": binding,
                       "launch": ("hip-graph replay (%d steps per graph launch)" % m["graph_steps"]) if a.graph else "eager",
                       "input_buffer_sets": n_sets,
                       "input_buffers_note": (("the steps rotate through %d copies of (x, grad), %.2f GB of inputs: reads come from HBM, "
                                               "not from the 256 MB Infinity Cache" % (n_sets, n_sets * set_bytes / 1e9))
                                              if n_sets * set_bytes >= (1 << 30) else
                                              ("the steps rotate through %d copies of (x, grad) (the cap), only %.2f GB of inputs: still partly "
                                               "cache-resident -- a launch-latency-bound workload either way" % (n_sets, n_sets * set_bytes / 1e9)))
                                             if n_sets > 1 else
                                             "one set of input buffers (%.2f GB per step streamed, beyond the 256 MB Infinity Cache)" % (5 * n_local * esz / 1e9)},
            "roofline": {"bound": "hbm", "kernel": "lsq::%s<%s> (fused dx + d_scale/d_shift reduction)" % (kb, io),
                         "achieved": round(bwd_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(bwd_gbs / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                         "traffic_over_algorithmic": (round(traffic / float(bytes_bwd * n_local), 5) if traffic else None),
                         "bytes_per_launch": bytes_bwd * n_local, "avg_launch_ms": round(bwd_avg, 5), "launches_timed": len(bwd_ms),
                         "median_launch_ms": round(bwd_ms[len(bwd_ms) // 2], 5),
                         "fwd": {"kernel": "lsq::%s<%s>" % (kf, io), "achieved": round(fwd_gbs, 1),
                                 "frac": round(fwd_gbs / HBM_PEAK_GBS, 4), "avg_launch_ms": round(fwd_avg, 5),
                                 "bytes_per_launch": bytes_fwd * n_local},
                         "step_achieved": round(step_gbs, 1), "step_frac": round(step_gbs / HBM_PEAK_GBS, 4),
                         # the read-only variant next to the all-traffic figure -- 3 of the 5
                         # algorithmic storage elements per element are reads (1 forward + 2 backward), so it is 0.6 x step_frac
                         "step_reads_only_achieved": round(step_gbs * 0.6, 1),
                         "step_reads_only_frac": round(step_gbs * 0.6 / HBM_PEAK_GBS, 4)},
        }
        if dumped is not None:
            line["dumped_outputs"] = {"dir": a.dump_outputs, "files": dumped}
        if world > 1 or a.assume_peers:
            line["config"]["collective"] = m["collective_route"] + (" (" + a.collective + ")" if a.assume_peers else "")
            if preflight:
                line["config"]["collective_preflight"] = dict(preflight)
            if m.get("verified"):
                line["config"]["collective_verified"] = m["verified"]["collective_verified"]
                line["parity_vs_reference"] = m["verified"]["parity_vs_reference"]
            if route_info[0]:
                line["config"]["communicator"] = route_info[0]
        if world > 1:
            # rank 0's shard step alone / the same step inside the N-rank job (barrier-bracketed, max over ranks): what the
            # collective and the co-running ranks cost one GPU.  1.0 = none.
            line["per_gpu_efficiency"] = round(m["solo_ms"] / (elapsed_max / a.steps * 1e3), 4)
            line["rank0_shard_alone_ms_per_step"] = round(m["solo_ms"], 5)
        if world == 1 and a.full and not a.no_yardstick:
            # Context for the roofline fraction, measured live on THIS box after the timed region: the framework's /
            # vendor's own kernels on the same two traffic shapes (ATen's vectorised add = 2 reads : 1 write like the
            # backward; its copy = 1 read : 1 write like the forward).  Not part of `value`.
            try:
                def _gbs(fn, bytes_per_elem):
                    reps = max(5, n_sets)
                    fn(0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for k in range(reps):
                        fn(k % n_sets)
                    e1.record()
                    e1.synchronize()
                    return round(bytes_per_elem * n_local / (e0.elapsed_time(e1) / reps * 1e-3) / 1e9, 1)
                scratch = torch.empty_like(x)
                line["roofline"]["same_box_reference_kernels"] = {
                    "aten_add_2r1w_GBps": _gbs(lambda k: torch.add(gs[k], xs[k], out=scratch), bytes_bwd),
                    "aten_copy_1r1w_GBps": _gbs(lambda k: scratch.copy_(xs[k]), bytes_fwd)}
                del scratch
            except Exception as e:      # context only: never let it break the bench line
                line["roofline"]["same_box_reference_kernels"] = {"error": repr(e)}
        sustained = None
        if world == 1 and a.workload == "cfg2" and not a.graph and a.full and not a.no_secondary and not (a.variant_fwd or a.variant_bwd):
            # The headline region is K steps (the driver's K = 20: 13 ms).  The SAME step, on the same buffers, for at least a
            # second, HIP events on 1 % of the steps: the sustained figure next to the burst.  DESIGN.md section 5 says which of
            # the two the 70 % claim rests on (both must clear it).
            try:
                per = elapsed_max / m["steps"]
                sus_steps = int(min(6000, max(300, -(-(1.1 / per) // 100) * 100)))       # >= 1.1 s of steps, a multiple of 100
                sm = measure("cfg2", sus_steps, 0, inputs=(m["xs"], m["gs"], m["scale"], m["shift"]), event_every=100)
                s_wall = sm["elapsed_max"] / sm["steps"]
                s_bwd = bytes_bwd * n_local / (sm["bwd_avg"] * 1e-3) / 1e9
                s_fwd = bytes_fwd * n_local / (sm["fwd_avg"] * 1e-3) / 1e9
                s_step = (bytes_fwd + bytes_bwd) * n_local / ((sm["fwd_avg"] + sm["bwd_avg"]) * 1e-3) / 1e9
                sustained = {"workload": "cfg2_sustained", "shape": sm["shape"], "storage": sm["dtype_name"], "steps": sm["steps"],
                             "wall_s": round(sm["elapsed_max"], 4), "value": round(n_local / s_wall / 1e9, 3), "unit": "GElem/s",
                             "ms_per_step": round(s_wall * 1e3, 5), "fwd_ms": round(sm["fwd_avg"], 5), "bwd_ms": round(sm["bwd_avg"], 5),
                             "bwd_frac": round(s_bwd / HBM_PEAK_GBS, 4), "fwd_frac": round(s_fwd / HBM_PEAK_GBS, 4),
                             "step_frac": round(s_step / HBM_PEAK_GBS, 4),
                             "step_frac_wall": round((bytes_fwd + bytes_bwd) * n_local / s_wall / 1e9 / HBM_PEAK_GBS, 4),
                             "events_on_steps": len(sm["bwd_ms"]), "launch": "eager", "host_binding": binding,
                             "what": "the headline step for >= 1 s on the headline's own buffers, HIP events on every 100th step"}
                line["roofline"]["sustained"] = {"achieved": round(s_bwd, 1), "frac": round(s_bwd / HBM_PEAK_GBS, 4),
                                                 "avg_launch_ms": round(sm["bwd_avg"], 5), "launches_timed": len(sm["bwd_ms"]),
                                                 "step_frac": round(s_step / HBM_PEAK_GBS, 4), "step_frac_wall": sustained["step_frac_wall"],
                                                 "steps": sm["steps"], "wall_s": sustained["wall_s"], "value": sustained["value"]}
                line["roofline"]["burst_vs_sustained"] = ("`frac` / `step_frac` above: the K timed steps of `value` (a burst when K is small); "
                                                          "`sustained`: the same step for >= 1 s -- the 70 % target is claimed on the LOWER of the two")
                del sm
            except Exception as e:      # context only
                sustained = {"workload": "cfg2_sustained", "error": repr(e)}
        if world == 1 and binding == "native" and not a.graph and a.full and not a.no_secondary:
            # north_star describes Python host code over the thin C ABI; the timed region above ran the C++ host binding (same C
            # entry points, less host time per call).  The same workload through the Python / ctypes host layer, 20 steps:
            try:
                # ... on the SAME input buffers as the timed region (the placement of a fresh 822 MB allocation moves config 2's
                # kernels by several % -- profiles/r04_buffer_offsets.txt -- which a host-layer comparison must not pick up), with
                # per-op events, and then the C++ binding again on those buffers for the same 20 steps: A / B / A
                same = (m["xs"], m["gs"], m["scale"], m["shift"])
                pm = measure(a.workload, 20, 5, ops=ops_of["ctypes"], inputs=same)
                nm = measure(a.workload, 20, 5, ops=ops_of["native"], inputs=same)
                line["config"]["python_ctypes_host_layer"] = {
                    "ms_per_step": round(pm["elapsed_max"] / pm["steps"] * 1e3, 5),
                    "value": round(pm["n_global"] * pm["steps"] / pm["elapsed_max"] / 1e9, 3), "steps": pm["steps"],
                    "fwd_ms": round(pm["fwd_avg"], 5), "bwd_ms": round(pm["bwd_avg"], 5),
                    "native_binding_same_buffers_same_steps": {
                        "ms_per_step": round(nm["elapsed_max"] / nm["steps"] * 1e3, 5),
                        "value": round(nm["n_global"] * nm["steps"] / nm["elapsed_max"] / 1e9, 3),
                        "fwd_ms": round(nm["fwd_avg"], 5), "bwd_ms": round(nm["bwd_avg"], 5)},
                    "ctypes_over_native": round(pm["elapsed_max"] / nm["elapsed_max"], 4),
                    "note": "torch.ops.torchlsq.* (torch.library registration in Python -> ctypes -> the same C ABI and kernels), "
                            "on the timed region's own input buffers; then the C++ binding again the same way"}
                del pm, nm, same
            except Exception as e:      # context only
                line["config"]["python_ctypes_host_layer"] = {"error": repr(e)}
        if world == 1 and a.full and not a.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(shape, a.workload)
        if world == 1 and a.workload == "cfg2" and not a.graph and a.full and not a.no_secondary:
            # The other single-GPU BASELINE configs (the small per-tensor one and the per-channel half of the path), timed in
            # this process right after the headline region, the same way: eager launches, rotated input buffers, per-op HIP
            # events.  `value` / `ms_per_step` are wall-clock over the K steps; the fractions are of the 8 TB/s peak.
            del xs, gs, x, m
            torch.cuda.empty_cache()
            t_sec = time.perf_counter()
            sec = []
            for w, extra in SECONDARY_RUNS:
                try:
                    name = extra.get("name", w)
                    mkw = {k: v for k, v in extra.items() if k in ("graph", "shard_of", "multi", "collective")}
                    sm = measure(w, a.secondary_steps if not extra.get("multi") else max(20, a.secondary_steps // 4), 20,
                                 warm_ms=60.0, extra_blocks=0 if mkw.get("graph") else 2, **mkw)
                    sb_f, sb_b = 2 * sm["esz"], 3 * sm["esz"]
                    rec = {"workload": name, "shape": sm["shape"], "storage": sm["dtype_name"],
                           "value": round(sm["n_global"] * sm["steps"] / sm["elapsed_max"] / 1e9, 3), "unit": "GElem/s",
                           "steps": sm["steps"], "ms_per_step": round(sm["elapsed_max"] / sm["steps"] * 1e3, 5),
                           "fwd_ms": round(sm["fwd_avg"], 5), "bwd_ms": round(sm["bwd_avg"], 5),
                           "bwd_frac": round(sb_b * sm["n_local"] / (sm["bwd_avg"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "fwd_frac": round(sb_f * sm["n_local"] / (sm["fwd_avg"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "step_frac": round((sb_f + sb_b) * sm["n_local"] / ((sm["fwd_avg"] + sm["bwd_avg"]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "step_frac_wall": round((sb_f + sb_b) * sm["n_local"] / (sm["elapsed_max"] / sm["steps"]) / 1e9 / HBM_PEAK_GBS, 4),
                           "launch": "graph" if sm["graph"] else "eager", "host_binding": binding, "input_buffer_sets": sm["n_sets"],
                           "blocks_ms_per_step": [round(tb / sm["steps"] * 1e3, 5) for tb in sm["block_times"]],
                           "value_is": "median of %d blocks of %d steps" % (len(sm["block_times"]), sm["steps"])}
                    if extra.get("note"):
                        rec["what"] = extra["note"]
                    if sm["graph"]:
                        rec["steps_per_graph_launch"] = sm["graph_steps"]
                        rec["per_op_ms_from"] = "a second, un-timed pass of eager launches (the ops are nodes of one graph launch)"
                    n_small = sm["n_local"] < (1 << 23) and not mkw
                    if mkw.get("collective"):
                        rec["collective"] = sm["collective_route"]
                        rec["communicator"] = route_info[0]
                        if sm.get("verified"):
                            rec["collective_verified"] = sm["verified"]["collective_verified"]
                            rec["parity_vs_reference"] = sm["verified"]["parity_vs_reference"]
                        solo = next((r_ for r_ in sec if r_.get("workload") == "cfg4_shard" and "ms_per_step" in r_), None)
                        if solo:
                            rec["wall_over_solo_shard_step"] = round(rec["ms_per_step"] / solo["ms_per_step"], 4)
                        del sm
                        # the same step through torch.distributed.all_reduce, and the HOST time of each form alone: the step on a
                        # tensor too small to keep the GPU busy ([1,16,14,14]: wall time per step = host time per step)
                        sm = measure(w, a.secondary_steps, 20, warm_ms=30.0, extra_blocks=2, shard_of=mkw["shard_of"], collective="c10d")
                        rec["ms_per_step_c10d"] = round(sm["elapsed_max"] / sm["steps"] * 1e3, 5)
                        rec["c10d_route_was"] = sm["collective_route"]
                        del sm
                        sm = measure(w, a.secondary_steps, 20, warm_ms=30.0, extra_blocks=2, shard_of=mkw["shard_of"], collective="native-inline")
                        rec["ms_per_step_native_inline"] = round(sm["elapsed_max"] / sm["steps"] * 1e3, 5)
                        rec["routes"] = ("native: reduction + rounding on the communicator's stream, ONE join of the compute stream at the end of the "
                                         "region (what hides the transport's latency at N > 1); native_inline: lsq_hip_comm_all_reduce in stream "
                                         "order (in a world of one it shows the call path's floor; at N > 1 the stream would sit out the "
                                         "all-reduce's latency every step); c10d: torch.distributed.all_reduce(async_op=True), waited a step later")
                        del sm
                        host = {}
                        for key, kw_ in (("shard_step_alone", {}), ("with_native_collective", {"collective": "native"}),
                                         ("with_c10d_collective", {"collective": "c10d"})):
                            hm = measure(w, a.secondary_steps, 20, warm_ms=20.0, extra_blocks=2, shard_of=mkw["shard_of"],
                                         shape_override=(1, 16, 14, 14), buffers=2, **kw_)
                            host[key] = round(hm["elapsed_max"] / hm["steps"] * 1e6, 2)
                            del hm
                        rec["host_us_per_step"] = host
                        rec["host_us_per_step_is"] = ("wall time per step of the same calls on a [1,16,14,14] tensor (3136 elements: the GPU "
                                                      "is never the bottleneck), eager, C++ host binding")
                        gpu_us = (rec["fwd_ms"] + rec["bwd_ms"]) * 1e3
                        rec["host_over_gpu_time"] = round(host["with_native_collective"] / gpu_us, 3) if gpu_us > 0 else None
                        sm = None
                    del sm
                    if n_small and binding == "native":
                        # launch-bound sizes: the Python / ctypes host layer next to the C++ binding (same kernels)
                        sm = measure(w, a.secondary_steps, 20, ops=ops_of["ctypes"], warm_ms=30.0)
                        rec["ms_per_step_ctypes_binding"] = round(sm["elapsed_max"] / sm["steps"] * 1e3, 5)
                        del sm
                    torch.cuda.empty_cache()
                    sec.append(rec)
                except Exception as e:      # never let a secondary record break the headline line
                    sec.append({"workload": extra.get("name", w), "error": repr(e)})
            if sustained is not None:
                sec.insert(0, sustained)
            line["secondary"] = sec
            line["secondary_wall_s"] = round(time.perf_counter() - t_sec, 2)
    strong = None
    if world > 1 and a.workload == "cfg2" and a.full and not a.no_secondary and 1024 % world == 0:
        try:
            # BASELINE config 4 next to the weak-scaled headline: [1024,1024,14,14] split over the ranks (STRONG scaling), the same
            # sharded step (every rank takes part: collectives inside)
            del xs, gs, x, m
            torch.cuda.empty_cache()
            m4 = measure("cfg4", a.steps, a.warmup)
            if rank == 0:
                t4 = m4["elapsed_max"] / m4["steps"]
                strong = {"workload": "cfg4: per-tensor quint8 float32 %s per GPU (global [1024,1024,14,14]), batch-sharded, "
                                      "1 RCCL all-reduce of fp64 [ds,db] per step" % m4["shape"],
                          "scaling": "strong", "value": round(m4["n_global"] / t4 / 1e9, 3), "unit": "GElem/s", "n_gpus": world,
                          "global_elements": m4["n_global"], "elements_per_gpu": m4["n_local"], "steps": m4["steps"],
                          "ms_per_step": round(t4 * 1e3, 5), "fwd_ms": round(m4["fwd_avg"], 5), "bwd_ms": round(m4["bwd_avg"], 5),
                          "step_frac_per_gpu": round(20.0 * m4["n_local"] / ((m4["fwd_avg"] + m4["bwd_avg"]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                          "rank0_shard_alone_ms_per_step": round(m4["solo_ms"], 5),
                          "per_gpu_efficiency": round(m4["solo_ms"] / (t4 * 1e3), 4), "input_buffer_sets": m4["n_sets"],
                          "collective": m4["collective_route"], "launch": "eager"}
                if m4.get("verified"):
                    strong["collective_verified"] = m4["verified"]["collective_verified"]
                    strong["parity_vs_reference"] = m4["verified"]["parity_vs_reference"]
            del m4
            # the same strong-scaled step over the OTHER routes of the collective (every rank runs the same sequence): which one the
            # transport between the GPUs favours is the one thing a single GPU cannot tell
            chosen = a.collective
            others = {}
            for route in ("native", "native-inline", "c10d"):
                if route == chosen or (route.startswith("native") and preflight and not preflight["ok"]):
                    continue
                a.collective = route
                mr = measure("cfg4", a.steps, a.warmup)
                if rank == 0:
                    tr = mr["elapsed_max"] / mr["steps"]
                    others[route] = {"ms_per_step": round(tr * 1e3, 5), "per_gpu_efficiency": round(mr["solo_ms"] / (tr * 1e3), 4),
                                     "collective": mr["collective_route"]}
                    if mr.get("verified"):
                        others[route]["collective_verified"] = mr["verified"]["collective_verified"]["ok"]
                        others[route]["parity_vs_reference"] = mr["verified"]["parity_vs_reference"]["ok"]
                del mr
            a.collective = chosen
            if rank == 0:
                strong["other_routes"] = others
        except Exception as e:      # the headline has been measured: an error here (every rank takes the same path) must not cost the line
            import traceback
            traceback.print_exc()
            strong = dict(strong or {}, error=repr(e))
    if rank == 0:
        if strong is not None:
            line["strong_scaled"] = strong
        try:                                   # whatever C stdio still holds goes where fd 1 points now: stderr
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        os.dup2(stdout_fd, 1)                  # the real stdout, for exactly one line
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)
    if preflight.get("hung"):
        os._exit(0)                            # a reduction that never ended sits on a stream: no orderly teardown with it
    if dist.is_initialized():
        from torchlsq import distributed as D
        D.destroy_native_comms()
        dist.destroy_process_group()
    return 0


def main():
    a = parse_args()
    if a.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))      # no launcher: this process only starts the ranks (it never touches the GPU)
    sys.exit(run_rank(a))


if __name__ == "__main__":
    main()
