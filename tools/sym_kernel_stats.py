"""Where a symmetric update's time goes, kernel by kernel -> profiles/sym_update_kernel_stats.txt.

Two kernel traces, one process per arm, then their comparison:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/default -o default -- python tools/sym_kernel_stats.py run
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/loss -o loss -- python tools/sym_kernel_stats.py run --symmetry loss
    python tools/sym_kernel_stats.py summarize DEFAULT_kernel_stats.csv LOSS_kernel_stats.csv [profiles/sym_update_kernel_stats.txt]
`run`: four iterations (OnPolicyRunner.learn(4): the graph captures and their dry runs included) of the registered GR1T1 task -- GR1T1CfgPPO
as it stands: 64 steps per env, 8 epochs x 25 minibatches, the 512-256-128 networks -- at 4096 envs, seed 1, with the flags that follow.
`summarize`: kernel time summed per kernel (every rocBLAS `Cijk_*` kernel under one name, every torch element-wise kernel under another),
sorted by what the second arm adds."""
import csv, sys; sys.path.insert(0, ".")


def run(flags):
    from wiki_grx_gym_amd.envs import GR1T1Cfg, GR1T1CfgPPO
    from wiki_grx_gym_amd.utils import get_args, task_registry
    args = get_args(["--task", "GR1T1", "--headless", "--num_envs", "4096", "--seed", "1", *flags])
    env, _ = task_registry.make_env("GR1T1", args=args, env_cfg=GR1T1Cfg())
    runner, _ = task_registry.make_alg_runner(env, name=None, args=args, train_cfg=GR1T1CfgPPO(), log_root=None)
    runner.learn(4)


def key(name):
    if name.startswith("Cijk"):
        return "rocBLAS GEMM kernels (Cijk_*), all"
    if "at::native" in name:
        return "torch element-wise / fill kernels, all"
    return name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60]


def load(path):
    d = {}
    for r in csv.DictReader(open(path)):
        c, t = d.get(key(r["Name"]), (0, 0))
        d[key(r["Name"])] = (c + int(r["Calls"]), t + int(r["TotalDurationNs"]))
    return d


def summarize(path_a, path_b, out):
    a, b = load(path_a), load(path_b)
    keys = sorted(set(a) | set(b), key=lambda k: -(b.get(k, (0, 0))[1] - a.get(k, (0, 0))[1]))
    lines = ["rocprofv3 --kernel-trace --stats of four iterations of the registered GR1T1 task (OnPolicyRunner.learn(4): 4096 envs, seed 1, 64 steps per env,",
             "8 epochs x 25 minibatches = 200 minibatch steps per iteration; graph capture and its dry runs included), one process per arm, one MI355X",
             "(tools/sym_kernel_stats.py): kernel time summed per kernel, the default against --symmetry loss (only the actor's rows double: 10485 -> 20970).",
             "Sorted by the difference.", "", f"{'kernel':62s} {'default calls':>13s} {'ms':>9s} {'loss calls':>11s} {'ms':>9s}"]
    for k in keys[:14]:
        lines.append(f"{k:62s} {a.get(k, (0, 0))[0]:13d} {a.get(k, (0, 0))[1] / 1e6:9.1f} {b.get(k, (0, 0))[0]:11d} {b.get(k, (0, 0))[1] / 1e6:9.1f}")
    tot = lambda d, i: sum(v[i] for v in d.values())
    lines.append(f"{'all kernels':62s} {tot(a, 0):13d} {tot(a, 1) / 1e6:9.1f} {tot(b, 0):11d} {tot(b, 1) / 1e6:9.1f}")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "run":
        run(sys.argv[2:])
    elif len(sys.argv) > 3 and sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "profiles/sym_update_kernel_stats.txt")
    else:
        sys.exit(__doc__)
