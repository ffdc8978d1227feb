"""What one observation-history push (--obs_history) costs: the HIP push (grx_obs_history_push, one launch) against the
torch spelling of the same definition (repeat + cat + where + copy) on the same tensors, at (4096, 39, H) and (4096, 168, H) for
H in {3, 6, 15}.  Per shape the two arms ALTERNATE in one process; a timed window is CALLS back-to-back pushes between two device
events (so a call's time is what the rollout pays: the larger of the host's enqueue and the device's work), REPEATS windows per arm
after a warm-up window, median and spread per call in microseconds.  Both arms' rows are compared (equal bytes) before they are timed.
    python tools/obs_history_time.py [repeats=31] [out=obs_history_step_time.json]   (the JSON line is printed too)"""
import json, statistics, sys; sys.path.insert(0, ".")
import torch
from wiki_grx_gym_amd.rl.history import ObsHistory
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 31
CALLS = 2000
DEV = "cuda:0"
assert torch.cuda.is_available(), "obs_history_time.py measures on the GPU: there is no fallback"


def arm(N, D, H, hip):
    h = ObsHistory(N, D, H, DEV)
    if not hip:
        h._hip = lambda x: False   # the torch spelling on the same device tensors
    return h


def window(h, x, dones):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        h.push(x, dones)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


rows = []
gen = torch.Generator().manual_seed(0)
for D in (39, 168):
    for H in (3, 6, 15):
        N = 4096
        x = torch.randn(N, D, generator=gen).to(DEV)
        dones = (torch.rand(N, generator=gen) < 0.02).to(DEV)     # about 2 % of the envs end per step, as in training
        arms = {"hip": arm(N, D, H, True), "torch": arm(N, D, H, False)}
        with torch.inference_mode():
            for h in arms.values():
                h.fill(x)
                for _ in range(3):
                    h.push(x + 1, dones)
            assert torch.equal(arms["hip"].current, arms["torch"].current), (N, D, H)
            ts = {k: [] for k in arms}
            for k, h in arms.items():
                window(h, x, dones)                               # warm-up
            for _ in range(repeats):
                for k, h in arms.items():
                    ts[k].append(window(h, x, dones))
        rows.append({"shape": [N, D, H], "bytes_moved": 2 * 4 * N * D * H,
                     "median_us_per_call": {k: round(statistics.median(v), 2) for k, v in ts.items()},
                     "min_max_us_per_call": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()}})
        print(rows[-1], flush=True)
out = {"what": "one observation-history push, HIP (one launch) against the torch spelling, alternated per shape", "device": torch.cuda.get_device_name(0),
       "calls_per_window": CALLS, "repeats": repeats, "dones_fraction": 0.02, "rows": rows}
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "obs_history_step_time.json", "w"), indent=1)
