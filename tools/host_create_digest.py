"""What grx_create PRODUCES, without a GPU: creates handles under one build of the library with the HIP runtime replaced by host memory
(tools/micro/hip_host_stub.cpp, built here on first use) and prints, per configuration, the kernel and launch geometry, grx_state_bytes, a hash
of the grx_save_state blob (header with the fingerprint + every state region), a hash of the tensor table and a hash of the sorted log of
uploaded tables.  Two builds that claim to build the same handles print the same lines: the check of a host-side refactor of grx_create
(profiles/r10_experiments.md).  usage: python tools/host_create_digest.py [path/to/libgrx_hip.so]"""
import ctypes as C, hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STUB = os.path.join(ROOT, "tools", "micro", "libhip_host_stub.so")
if not os.path.exists(STUB) or os.path.getmtime(STUB) < os.path.getmtime(STUB[:-3].replace("libhip", "hip") + ".cpp"):
    subprocess.run(["g++", "-O1", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-o", STUB, os.path.join(ROOT, "tools", "micro", "hip_host_stub.cpp")], check=True)
stub = C.CDLL(STUB, mode=C.RTLD_GLOBAL)   # ahead of the library: its hip* calls bind here
import numpy as np
from tests.helpers import make_cfg, make_terrain
from wiki_grx_gym_amd import _capi
from wiki_grx_gym_amd.envs import build_config

lib = C.CDLL(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "wiki-grx-gym_amd", "csrc", "libgrx_hip.so"))
api = _capi.bind(lib, "grx_")

CASES = [
    ("default", {}, dict(terrain="heightfield"), 4096, None),
    ("quad waves 4", {"GRX_QUAD_WAVES": "4"}, dict(terrain="heightfield"), 4096, None),
    ("lanes 2", {"GRX_LANES_PER_ENV": "2"}, dict(terrain="heightfield"), 4096, None),
    ("waves 1", {"GRX_WAVES_PER_BLOCK": "1"}, dict(terrain="heightfield"), 4096, None),
    ("32768", {}, dict(terrain="heightfield"), 32768, None),
    ("plane", {}, dict(terrain="plane"), 4096, None),
    ("trimesh", {}, dict(terrain="trimesh"), 4096, None),
    ("no dr no noise", {}, dict(terrain="heightfield", noise=False, dr=False), 1000, None),
    ("GR1T2", {}, dict(terrain="heightfield", task="GR1T2"), 4096, None),
    ("full", {}, dict(terrain="heightfield", task="GR1T1Full"), 4096, None),
    ("full g8", {"GRX_TREE_G": "8"}, dict(terrain="heightfield", task="GR1T1Full"), 4096, None),
    ("full generic", {"GRX_TREE": "0"}, dict(terrain="heightfield", task="GR1T1Full"), 4096, None),
    ("full trimesh", {}, dict(terrain="trimesh", task="GR1T1Full"), 4096, None),
    ("full plane", {}, dict(terrain="plane", task="GR1T1Full"), 4096, None),
    ("full 16384", {}, dict(terrain="heightfield", task="GR1T1Full"), 16384, None),
    ("force generic", {"GRX_FORCE_GENERIC": "1"}, dict(terrain="heightfield"), 4096, None),
    ("every_step", {}, dict(terrain="heightfield"), 4096, "every_step"),
    ("on_refresh", {}, dict(terrain="heightfield"), 4096, "on_refresh"),
    ("never", {}, dict(terrain="heightfield"), 4096, False),
    ("full on_refresh", {}, dict(terrain="heightfield", task="GR1T1Full"), 4096, "on_refresh"),
    ("full generic on_refresh", {"GRX_TREE": "0"}, dict(terrain="heightfield", task="GR1T1Full"), 4096, "on_refresh"),
    ("full every_step", {}, dict(terrain="heightfield", task="GR1T1Full"), 4096, "every_step"),
]
for label, env, kw, N, publish in CASES:
    for k in ("GRX_QUAD_WAVES", "GRX_LANES_PER_ENV", "GRX_WAVES_PER_BLOCK", "GRX_TREE_G", "GRX_TREE", "GRX_FORCE_GENERIC"):
        os.environ.pop(k, None)
    os.environ.update(env)
    kw = dict(dict(noise=True, dr=True, push=True), **kw)
    cfg = make_cfg(**kw)
    if publish is not None:
        cfg.env.publish_rigid_body_states = publish
        if publish:
            cfg.env.publish_measured_heights = publish
    ter = make_terrain(cfg, N, 1)
    c, keep, _ = build_config.build(cfg, cfg.sim.dt, N, terrain=ter)
    stub.stub_reset()
    h = C.c_void_p()
    rc = api["create"](C.byref(c), 0, C.byref(h))
    if rc:
        print(label, "create failed", rc, api["last_error"]()); continue
    li = _capi.LayoutInfo(); api["layout"](h, C.byref(li))
    nb = C.c_int64(0); api["state_bytes"](h, C.byref(nb))
    buf = np.empty(nb.value, dtype=np.uint8)
    rc = api["save_state"](h, buf.ctypes.data, nb.value, None)
    descs = []
    for name, tid in sorted(_capi.T.items(), key=lambda kv: kv[1]):
        d = _capi.TensorDesc()
        r = api["tensor"](h, tid, C.byref(d))
        descs.append((name, r, bool(d.data), d.dtype, d.ndim, tuple(d.shape), tuple(d.stride)) if r == 0 else (name, r))
    out = (C.c_uint64 * 4096)()
    n = stub.stub_log(out, 4096)
    log = sorted((out[i], out[i + 1]) for i in range(0, n, 2))
    print(label, "|", li.kernel.decode(), li.lanes_per_env, li.waves_per_block, li.envs_per_block, li.num_blocks, "| state_bytes", nb.value, "save rc", rc,
          "blob", hashlib.sha256(buf.tobytes()).hexdigest()[:16], "| descs", hashlib.sha256(repr(descs).encode()).hexdigest()[:16],
          "| uploads", len(log), hashlib.sha256(repr(log).encode()).hexdigest()[:16], flush=True)
    api["destroy"](h)
