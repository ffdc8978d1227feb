"""What the two HIP entry points of policy distillation (--distill_from) cost against their torch spellings on the same
tensors: the behaviour loss with its gradient (grx_distill_loss, two launches, against torch's mse_loss / huber_loss + autograd backward)
at (4096 * 24 / 4, 10), a minibatch of the GR1T1 train shape, and the per-step store (grx_distill_store, one launch, against three
copy_ calls and the episode bookkeeping in torch) at (4096, 39 * H, 10) for H in {1, 15}.  Per shape the two arms ALTERNATE in one
process; a timed window is CALLS back-to-back calls between two device events (so a call's time is what training pays: the larger of
the host's enqueue and the device's work), REPEATS windows per arm after a warm-up window, median and spread per call in microseconds.
Both arms' results are compared before they are timed: the store's rows byte for byte, the loss and its gradient inside the bounds of
tests/distill_ref.py.  The loss rows have a third arm, the C entry point alone on preallocated outputs: "hip" and "torch" both go through
torch's autograd engine (forward, backward), whose host time is most of their call.  Also recorded: the peak error of both losses
against float64, in ulp of the loss, over the shapes of tests/test_distill_gpu.py.
    python tools/distill_time.py [repeats=31] [out=profiles/distill_step_time.json]   (the JSON line is printed too)"""
import ctypes as C, json, statistics, sys; sys.path.insert(0, ".")
import numpy as np
import torch
from tests import distill_ref as R
from wiki_grx_gym_amd.rl import distillation as D
from wiki_grx_gym_amd.rl.fused_loss import load_ppo_library
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 31
CALLS = 2000
DEV = "cuda:0"
assert torch.cuda.is_available(), "distill_time.py measures on the GPU: there is no fallback"


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def measure(arms):
    ts = {k: [] for k in arms}
    for fn in arms.values():
        window(fn)                                                # warm-up
    for _ in range(repeats):
        for k, fn in arms.items():
            ts[k].append(window(fn))
    return {"median_us_per_call": {k: round(statistics.median(v), 2) for k, v in ts.items()},
            "min_max_us_per_call": {k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()}}


rows = []
# ---- the loss and its gradient ----------------------------------------------------------------------------------------------------------
B, A = 4096 * 24 // 4, 10
for loss_type in R.LOSSES:
    s_np, t_np = R.loss_inputs(B, A)
    want, want_grad = R.loss_and_grad(s_np, t_np, loss_type)
    s, t = torch.tensor(s_np).to(DEV).requires_grad_(True), torch.tensor(t_np).to(DEV)

    def step(fused):
        s.grad = None
        loss = D.distill_loss(s, t, loss_type, fused=fused)
        loss.backward()
        return loss
    for fused in (True, False):
        loss = step(fused)
        assert abs(float(loss) - want) <= (B * A + 2) * 2.0 ** -24 * want, (loss_type, fused)
        assert (np.abs(s.grad.cpu().numpy().astype(np.float64) - want_grad) <= R.grad_bound(want_grad)).all(), (loss_type, fused)
    # ... and the entry point alone, on preallocated outputs: what is left of "hip" without torch's autograd engine around it
    lib, sd = load_ppo_library(), s.detach()
    out, d_mu = torch.empty(1, device=DEV), torch.empty_like(sd)
    part = torch.empty(lib.grx_distill_loss_partials_size(B, A), device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    entry = lambda: lib.grx_distill_loss(B, A, sd.data_ptr(), t.data_ptr(), int(loss_type == "huber"), out.data_ptr(), d_mu.data_ptr(), part.data_ptr(), stream)
    assert entry() == 0 and torch.equal(out[0], step(True).detach()) and torch.equal(d_mu, s.grad)
    rows.append({"what": "loss + gradient", "loss": loss_type, "shape": [B, A], "bytes_moved": 3 * 4 * B * A,
                 **measure({"hip": lambda: step(True), "torch": lambda: step(False), "hip_entry_alone": entry})})
    print(rows[-1], flush=True)

# ---- the store ---------------------------------------------------------------------------------------------------------------------------
N = 4096
for H in (1, 15):
    Dm = 39 * H
    obs, labels, rewards, dones, log = R.store_inputs(N, Dm, A, "mixed")
    dones = np.arange(N) % 50 == 0                                  # about 2 % of the envs end per step, as in training
    dev = lambda a: torch.tensor(a).to(DEV)
    arms, state = {}, {}
    for name, store in (("hip", D.store_hip), ("torch", D.store_torch)):
        st, tlog = D.DistillStorage(N, 2, Dm, A, DEV), tuple(dev(a) for a in log)
        args = (st, 1, dev(obs), dev(labels), dev(dones), dev(rewards), tlog)
        store(*args)
        state[name] = [x.cpu().numpy().tobytes() for x in (st.observations, st.labels, st.dones, *tlog)]
        arms[name] = (lambda store=store, args=args: store(*args))
    assert state["hip"] == state["torch"], (N, Dm, A)
    with torch.inference_mode():
        rows.append({"what": "store", "shape": [N, Dm, A], "bytes_moved": 2 * (4 * N * (Dm + A) + N) + 5 * 4 * N, **measure(arms)})
    print(rows[-1], flush=True)

# ---- the loss's error against float64 over the test shapes -------------------------------------------------------------------------------
peaks = {}
for loss_type in R.LOSSES:
    worst = {"hip": 0.0, "torch": 0.0}
    for batch in (1, 63, 64, 65, 256, 257, 4099):
        for A_ in (1, 10, 32):
            s_np, t_np = R.loss_inputs(batch, A_)
            want, _ = R.loss_and_grad(s_np, t_np, loss_type)
            s, t = torch.tensor(s_np).to(DEV), torch.tensor(t_np).to(DEV)
            ulp = float(np.spacing(np.float32(want)))
            for k, fused in (("hip", True), ("torch", False)):
                worst[k] = max(worst[k], abs(float(D.distill_loss(s, t, loss_type, fused=fused)) - want) / ulp)
    peaks[loss_type] = {k: round(v, 3) for k, v in worst.items()}
print("loss error peaks [ulp]:", peaks, flush=True)

out = {"what": "policy distillation: the HIP loss (+ gradient) and store against their torch spellings, alternated per shape",
       "device": torch.cuda.get_device_name(0), "calls_per_window": CALLS, "repeats": repeats, "rows": rows,
       "loss_error_peaks_ulp": {"shapes": "batch in {1, 63, 64, 65, 256, 257, 4099} x A in {1, 10, 32}", **peaks}}
print(json.dumps(out))
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "profiles/distill_step_time.json", "w"), indent=1)
