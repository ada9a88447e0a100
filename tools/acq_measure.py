"""Measurement of the acquisition search on the GPU (log in profiles/acquire/):
device-event time of one gss_acquire_device call (all its kernels: maxima, replicas, wipe-off,
correlator, peaks) for the default search at two rates, the matrix-core correlator against the
VALU form (GSS_ACQ_PATH=valu), each in processes of its own, alternating.  A process warms up,
then times 5 samples of REPS back-to-back calls between two events; the line gives the median
per call.  The int8 MAC rate counts the multiply-adds of the definition, n_prn * bins * T * M * L
* 2 (I and Q); LDS bytes per MAC are counted from the kernel's tile shape, not measured.

usage: python tools/acq_measure.py [--rounds 3]      (a GPU is required)
       python tools/acq_measure.py --child <shape index> <mfma|valu>"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))

# (label, fs, PRNs): +-10 kHz at 500 Hz, 1 ms x 10
SHAPES = [("2.6 MS/s, 32 PRNs", 2600000, list(range(1, 33))),
          ("20 MS/s, 8 PRNs", 20000000, [1, 3, 6, 9, 12, 17, 23, 28])]
REPS = {0: 20, 1: 4}


def clocks():
    """the GPU's current clocks as rocm-smi shows them (read only); '' if it cannot say"""
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True,
                             text=True, timeout=30).stdout
        keep = [ln.split(":", 1)[1].strip() for ln in out.splitlines()
                if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep)
    except Exception as e:                             # noqa: BLE001
        return f"(rocm-smi: {e})"


def child(si, path):
    import numpy as np
    import torch
    import gpssim_amd as G
    if path == "valu":
        os.environ["GSS_ACQ_PATH"] = "valu"
    else:
        os.environ.pop("GSS_ACQ_PATH", None)
    label, fs, prns = SHAPES[si]
    acq = G.Acq(fs, 16, 1, 10, 500, 20, -1, prns)
    L, T, N, E, P = acq.sizes()
    dev = G.Device(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.randint(-3000, 3001, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
    peaks = torch.zeros(32 * P, dtype=torch.uint8, device="cuda")
    sh = torch.zeros(1, dtype=torch.int32, device="cuda")
    reps = REPS[si] if path == "mfma" else max(1, REPS[si] // 4)
    for _ in range(3):                                  # warm-up: code objects, scratch, clocks
        dev.acquire(acq, x.data_ptr(), peaks.data_ptr(), 0, sh.data_ptr())
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            dev.acquire(acq, x.data_ptr(), peaks.data_ptr(), 0, sh.data_ptr())
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    med = float(np.median(ms))
    macs = P * 41 * T * 10 * L * 2
    digest = int(np.bitwise_xor.reduce(peaks.cpu().numpy().view(np.uint64)))
    print(f"{label:18s} {path:4s}: median {med:8.3f} ms per call (min {min(ms):.3f}, max "
          f"{max(ms):.3f}; {reps} calls per sample), {macs / med / 1e9:8.1f} T int8 MAC/s, "
          f"peaks xor {digest:016x}, shift {int(sh.item())}", flush=True)
    dev.close()


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), sys.argv[3])
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
    print("clocks before:", clocks(), flush=True)
    for si in range(len(SHAPES)):
        for _ in range(rounds):
            for path in ("mfma", "valu"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(si),
                                    path], timeout=600)
                if r.returncode != 0:                   # nothing more on the GPU after a failure
                    sys.exit(f"child {si} {path} failed with status {r.returncode}")
        print("clocks now:", clocks(), flush=True)


if __name__ == "__main__":
    main()
