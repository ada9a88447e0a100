"""The impair kernel's time per headline window (2,999 blocks x 260,000 samples) at each format
for the library GSS_LIB_PATH names (else the in-tree build), e.g. the table from LDS against
the table from global memory (tools/ablate.sh imp_l2 "-DGSS_IMP_TBL_L2"; profiles/impair/).

usage: [GSS_LIB_PATH=... GSS_ALLOW_LIB_OVERRIDE=1] python tools/impair_kernel_time.py TAG"""
import hashlib, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import numpy as np
import torch
import gpssim_amd as G
N = 2999 * 260000
dev = G.Device(0)
g = torch.Generator(device="cuda"); g.manual_seed(1)
iq = torch.randint(-1400, 1401, (2 * N,), dtype=torch.int16, device="cuda", generator=g)
out = torch.empty(4 * N, dtype=torch.uint8, device="cuda")
imp = G.Impair(410441, 0, 7)
st = torch.cuda.current_stream().cuda_stream
tag = sys.argv[1]
for fmt in (16, 8, 1):
    times = []
    for rep in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dev.impair_device(imp, iq.data_ptr(), 0, N, fmt, out.data_ptr(), stream=st)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    t = sorted(times[1:])
    h = hashlib.sha256(out[:1 << 24].cpu().numpy().tobytes()).hexdigest()[:12]
    print(f"{tag:8} -b {fmt:<2}: median {t[2]:.3f} ms min {t[0]:.3f} max {t[-1]:.3f}  out {h}", flush=True)
dev.close()
