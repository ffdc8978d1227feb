"""What profiles/beta_policy_parity.json records for the Beta policy's kernels, on one MI355X:
  functions_max_error_fp32_ulps: the largest error of grx_beta_functions' lgamma, digamma and trigamma against float64, in fp32 ulps of the
    float64 value, over tests/beta_ref.py::function_grid (4096 log-spaced points in [1, 1e4], 1, 2 and the integers up to 64), and where.
    tests/test_beta_policy_gpu.py asserts twice these figures.
  loss: per case of tests/beta_ref.py::LOSS_CASES, the largest error / tolerance per output tensor of grx_ppo_loss_beta against float64,
    beside the fp32 torch spelling's on the CPU for the same data (the tolerances take twice the figures just measured).
    python tools/beta_policy_parity.py [out=profiles/beta_policy_parity.json]"""
import json, os, sys; sys.path.insert(0, ".")
import torch
from tests import beta_ref as R
from wiki_grx_gym_amd.rl import beta as B

DEV = "cuda:0"
out_path = sys.argv[1] if len(sys.argv) > 1 else R.PARITY_JSON
assert torch.cuda.is_available(), "beta_policy_parity.py measures on the GPU: there is no fallback"
t = R.function_grid()
got = dict(zip(("lgamma", "digamma", "trigamma"), (o.cpu() for o in B.beta_functions(t.to(DEV)))))
ref = R.function_refs(t)
functions, where = {}, {}
for name in got:
    err = R.ulp_errors(got[name], ref[name])
    i = int(err.argmax())
    functions[name], where[name] = round(float(err[i]), 4), float(t[i])
    print(name, functions[name], "ulps at", where[name], flush=True)
fn = {k: 2.0 * v for k, v in functions.items()}
rows = []
for Bn, A, setting, use_clipped in R.LOSS_CASES:
    d = R.loss_case(Bn, A, setting)
    r64 = R.loss64(*d, R.CLIP, R.VCOEF, R.ECOEF, use_clipped)
    tol = R.tolerances(d, r64, fn)
    dd = tuple(x.to(DEV) for x in d)
    raw, value = dd[0].clone().requires_grad_(), dd[1].clone().requires_grad_()
    o = B.fused_ppo_loss_beta(raw, value, *dd[2:], R.CLIP, R.VCOEF, R.ECOEF, use_clipped)
    o[2].backward()
    rnd = lambda e: {k: ([round(x, 4) for x in v] if isinstance(v, list) else round(v, 4)) for k, v in e.items()}
    rows.append({"batch": Bn, "actions": A, "setting": setting, "use_clipped_value_loss": use_clipped,
                 "kernel_error_over_tolerance": rnd(R.loss_errors(o.detach(), raw.grad, value.grad, r64, tol)),
                 "fp32_torch_cpu_error_over_tolerance": rnd(R.loss_errors(*R.torch_fp32_loss(d, use_clipped), r64, tol))})
    print(rows[-1], flush=True)
doc = {"what": "tools/beta_policy_parity.py on one MI355X", "functions_max_error_fp32_ulps": functions, "functions_worst_argument": where,
       "grid": "4096 log-spaced points in [1, 1e4], 1, 2, the integers up to 64; float64 reference: torch.lgamma / digamma / polygamma on the CPU",
       "loss": rows}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps(doc["functions_max_error_fp32_ulps"]))
