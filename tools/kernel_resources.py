"""Register / scratch / LDS budget of every kernel in a built library, from the code objects embedded in it.

    python tools/kernel_resources.py [wiki-grx-gym_amd/csrc/libgrx_hip.so] [--json profiles/rNN_kernel_resources.json]
    python tools/kernel_resources.py LIB [LIB ...] --code-hashes profiles/rNN_kernel_code.json
    python tools/kernel_resources.py --compare BEFORE.json AFTER.json      (exit status 1 when a kernel differs)

Walks the __CLANG_OFFLOAD_BUNDLE__ containers of the .so, takes every gfx950 code object and reads the AMDGPU metadata notes
(llvm-readelf --notes): vgpr / agpr counts, spilled VGPRs, private segment (scratch) bytes per lane, LDS bytes.  The numbers
VERDICT r3 asked to drive to zero -- `vgpr_spill_count`, `private_segment_fixed_size` of the step kernels -- come from here.

--code-hashes: for a host-side refactor, the proof that the device code is unchanged KERNEL BY KERNEL.  A library's bytes move when the host
code merely instantiates the kernels in another order; a function's own bytes do not.  Per gfx950 code object and mangled name: the sha256 of
every FUNC symbol's bytes, every kernel descriptor (.kd) outside its code-entry offset (bytes 16-23), and the resource rows above."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
DEMANGLE = "c++filt"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob):
    pos = 0
    while True:
        pos = blob.find(MAGIC, pos)
        if pos < 0:
            return
        n, = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[pos + off:pos + off + size]
        pos += len(MAGIC)


def kernels_of(co_bytes):
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(co_bytes)
        path = f.name
    try:
        txt = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
    finally:
        os.unlink(path)
    out = []
    for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
        blk = ".agpr_count:" + blk
        g = lambda key: (re.search(r"\." + key + r":\s+(\S+)", blk) or [None, None])[1]
        sym = g("name")
        name = subprocess.run([DEMANGLE, sym], capture_output=True, text=True).stdout.strip() if sym else "?"
        name = re.sub(r"\(anonymous namespace\)::", "", name).split("(")[0].replace("void ", "")
        out.append({"kernel": name, "vgpr": int(g("vgpr_count")), "agpr": int(g("agpr_count")), "sgpr": int(g("sgpr_count")),
                    "vgpr_spill": int(g("vgpr_spill_count")), "sgpr_spill": int(g("sgpr_spill_count")),
                    "scratch_bytes": int(g("private_segment_fixed_size")), "lds_bytes": int(g("group_segment_fixed_size")),
                    "max_flat_workgroup_size": int(g("max_flat_workgroup_size"))})
    return out


def code_hashes(co_bytes):
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(co_bytes)
        path = f.name
    try:
        txt = subprocess.run([READELF, "-S", "-s", "-W", path], capture_output=True, text=True, check=True).stdout
    finally:
        os.unlink(path)
    sec = {int(m[1]): (int(m[2], 16), int(m[3], 16)) for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", txt, re.M)}   # index -> (address, offset)
    funcs, kds = {}, {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", txt, re.M):
        value, size, kind, ndx, name = int(m[1], 16), int(m[2]), m[3], int(m[4]), m[5]
        addr, off = sec[ndx]
        data = co_bytes[off + value - addr:off + value - addr + size]
        if kind == "FUNC":
            funcs[name] = hashlib.sha256(data).hexdigest()
        elif name.endswith(".kd") and size == 64:
            kds[name] = (data[:16] + bytes(8) + data[24:]).hex()
    return {"functions": funcs, "descriptors": kds, "resources": sorted(kernels_of(co_bytes), key=lambda r: r["kernel"])}


def compare(before, after):
    a, b = json.load(open(before)), json.load(open(after))
    bad = 0
    for lib in sorted(set(a) | set(b)):
        cos_a, cos_b = a.get(lib, []), b.get(lib, [])
        if len(cos_a) != len(cos_b):
            print(f"{lib}: {len(cos_a)} code objects before, {len(cos_b)} after"); bad += 1
        nfun = 0
        for i, (x, y) in enumerate(zip(cos_a, cos_b)):
            for part in ("functions", "descriptors"):
                for name in sorted(set(x[part]) | set(y[part])):
                    if x[part].get(name) != y[part].get(name):
                        print(f"{lib} code object {i}: {part[:-1]} {name} {'differs' if name in x[part] and name in y[part] else 'is in one listing only'}"); bad += 1
            if x["resources"] != y["resources"]:
                print(f"{lib} code object {i}: resource rows differ"); bad += 1
            nfun += len(y["functions"])
        print(f"{lib}: {len(cos_b)} code objects, {nfun} functions compared")
    print(f"{bad} differing kernels")
    return 1 if bad else 0


def main():
    argv = list(sys.argv[1:])
    if "--compare" in argv:
        i = argv.index("--compare")
        sys.exit(compare(argv[i + 1], argv[i + 2]))
    if "--code-hashes" in argv:
        i = argv.index("--code-hashes"); out = argv[i + 1]; del argv[i:i + 2]
        listing = {os.path.basename(lib): [code_hashes(co) for co in code_objects(open(lib, "rb").read())] for lib in argv}
        with open(out, "w") as f:
            json.dump(listing, f, indent=1, sort_keys=True)
        for lib, cos in listing.items():
            print(f"{lib}: {len(cos)} gfx950 code objects, {[len(c['descriptors']) for c in cos]} kernels, {sum(len(c['functions']) for c in cos)} functions")
        return
    out_json = None
    if "--json" in argv:
        i = argv.index("--json"); out_json = argv[i + 1]; del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    lib = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wiki-grx-gym_amd", "csrc", "libgrx_hip.so")
    rows = []
    for co in code_objects(open(lib, "rb").read()):
        rows += kernels_of(co)
    rows.sort(key=lambda r: r["kernel"])
    print(f"{'kernel':58s} vgpr agpr spill scratch    lds")
    for r in rows:
        print(f"{r['kernel'][:58]:58s} {r['vgpr']:4d} {r['agpr']:4d} {r['vgpr_spill']:5d} {r['scratch_bytes']:7d} {r['lds_bytes']:6d}")
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"library": os.path.basename(lib), "kernels": rows}, f, indent=1)


if __name__ == "__main__":
    main()
