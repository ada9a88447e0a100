"""Times gss_obs_device: one form of the kernel per process (GSS_OBS_PATH), device
events around whole calls, the median of 5 after a warm-up, at 12 jobs x 30,000 and 12 x 300,000
records with instants at 10 Hz and at every epoch; and gss_obs_host on 16 threads over the same
input.  Prints one JSON line per shape.  Run it once per form, alternating:
    for i in 1 2 3; do python tools/obs_measure.py fast; python tools/obs_measure.py plain; done
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    form = sys.argv[1] if len(sys.argv) > 1 else "fast"
    if form == "plain":
        os.environ["GSS_OBS_PATH"] = "plain"
    else:
        os.environ.pop("GSS_OBS_PATH", None)
    import numpy as np
    import torch
    import gpssim_amd as G
    fs, jobs = 1000000, 12
    dev = G.Device(0)
    for n_rec in (30000, 300000):
        # records of a steady loop: 1000 samples an epoch, Doppler and code step as tracking
        # leaves them (the values do not change the work)
        rec = np.zeros((jobs, n_rec), G.TRK_REC_DTYPE)
        rng = np.random.default_rng(n_rec)
        for j in range(jobs):
            rec["s"][j] = 37 * j + 1000 * np.arange(n_rec, dtype=np.int64)
            rec["w"][j] = rng.integers(-2**24, 2**24)
            rec["dcs"][j] = 0
        count = np.full(jobs, n_rec, np.int32)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        d_count = torch.from_numpy(count).cuda()
        for what, step in (("10 Hz", fs // 10), ("every epoch", 1000)):
            n_fix = (n_rec * 1000) // step
            d_obs = torch.zeros(32 * jobs * n_fix, dtype=torch.uint8, device="cuda")
            ms = []
            for it in range(6):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dev.observables(fs, d_rec.data_ptr(), n_rec, d_count.data_ptr(), jobs, 0, step,
                                n_fix, d_obs.data_ptr())
                b.record()
                torch.cuda.synchronize()
                if it:
                    ms.append(a.elapsed_time(b))
            got = d_obs.cpu().numpy().view(G.OBS_DTYPE).reshape(jobs, n_fix)
            hs = []
            for it in range(6):
                t0 = time.perf_counter()
                want = G.observables_host(fs, rec, count, 0, step, n_fix, threads=16)
                if it:
                    hs.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"form": form, "records": n_rec, "instants": what, "n_fix": n_fix,
                              "device_ms_median": round(float(np.median(ms)), 4),
                              "device_ms": [round(x, 4) for x in ms],
                              "host16_ms_median": round(float(np.median(hs)), 4),
                              "upload_MB": round(rec.nbytes / 1e6, 1),
                              "equal": bool(np.array_equal(got, want))}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
