"""Time of the PPO policy head on synthetic features (EXPERIMENTS.md "PPO policy head"); no simulator, no extractor.

  (a) ppo_loss forward + backward at B = 512, F = 256, pi = vf = [256, 256], A = 7: one PPO minibatch behind the extractor (ppo_mae.py:280-340)
  (b) act under no_grad at B = 8: the head of one environment step (MAEPolicy.forward, pretrain_models.py:899-923)

each on two paths on the same GPU:
  hip    m3l_amd.ActorCriticHead (m3l_amd/csrc/policy.hip)
  eager  the float32 torch restatement of the same arithmetic (tests/ppo_cases.py: nn.functional.linear, tanh, torch.distributions.Normal, the
         loss lines of ppo_mae.py, autograd): what a user of the reference runs today
and, for (a), with and without the reads of the logged statistics: the reference reads five scalars one by one (`.item()` / `.cpu()`,
ppo_mae.py:297, 298, 312, 321, 331), the HIP path reads its five-float statistics tensor in one copy (`stats_dict`).

Per path:
  call_us     time per call from device events around a window of back-to-back calls that ends in a synchronise.  The paths are timed in
              alternating windows (hip, eager, hip + read, eager + read, and again; --rounds of them, --iters calls each for (a), ten times that for
              (b), so a window lasts from half a second to a few seconds); reported: the median window and the minimum and maximum over the windows
  host_us     host clock around the same window up to, not including, its synchronise: the enqueue time per call (with reads it contains the waits
              of those reads); median, minimum, maximum likewise
  entry_points   (hip) device time per C entry point from the library's event brackets (m3l_prof_*), in a loop of its own; an empty bracket is
              part of each figure
  kernel_us / launches / copies   from torch.profiler (roctracer's kernel records) over 10 calls in a run of its own, because tracing slows the
              host: summed device time of the kernels, number of kernels and of memory copies per call.  These are not rocprofv3 figures.
Both paths' losses are printed, so that a wrong result cannot pass as a fast one.  Without a GPU the tool fails; it has no fallback.

Usage: python tools/policy_head_bench.py [--iters 1500] [--rounds 5] [--warmup 50]   (one JSON line on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ppo_cases as PC  # noqa: E402
import m3l_amd  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
ARCH = (256, (256, 256), (256, 256), 7)


def window(fn, iters):
    """One timed window of `iters` back-to-back calls -> (device-event µs per call, host-clock µs per call before the synchronise, last result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, host / iters * 1e6, out


def alternate(fns, iters, warmup, rounds):
    """Times the paths of `fns` ({name: fn}) in `rounds` alternating windows (a b c d a b c d ...), each of `iters` calls after `warmup` calls of
    every path: per path the median, minimum and maximum over its windows, so a drift of the box shows as spread, not as a difference."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    call, host, last = {n: [] for n in fns}, {n: [] for n in fns}, {}
    for _ in range(rounds):
        for n, fn in fns.items():
            c, h, last[n] = window(fn, iters)
            call[n].append(c)
            host[n].append(h)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return {n: {"call_us": round(med(call[n]), 1), "call_us_min_max": [round(min(call[n]), 1), round(max(call[n]), 1)], "host_us": round(med(host[n]), 1),
                "host_us_min_max": [round(min(host[n]), 1), round(max(host[n]), 1)], "window_calls": iters, "windows": rounds} for n in fns}, last


def traced(fn, iters=10):
    """Kernels and copies per iteration and their summed device time, from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    dev_us = 0.0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            if e.name.lower().startswith(("memcpy", "memset")):
                copies += 1
            else:
                kernels += 1
                dev_us += float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
    return {"launches": round(kernels / iters, 1), "copies": round(copies / iters, 1), "kernel_us": round(dev_us / iters, 1)}


def entry_points(fn, iters=50):
    """Device time per C entry point from the library's own event brackets (m3l_prof_*), in a loop of its own."""
    lib = L.lib()
    lib.m3l_prof_begin(None, 1)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    lib.m3l_prof_end()
    out = {}
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        ms, n, w, b = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(b))
        if n.value:
            out[name.value.decode()] = {"us_per_call": round(ms.value / n.value * 1e3, 1), "calls_per_iter": round(n.value / iters, 2)}
    return out


def counted(fn):
    try:
        return traced(fn)
    except Exception as e:      # noqa: BLE001  (a profiler that does not start leaves the counts unmeasured, the timings stand)
        return {"launches": "not measured", "copies": "not measured", "kernel_us": "not measured", "profiler_error": repr(e)[:200]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1500, help="calls per timed window of (a); (b) takes ten times as many")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per path")
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("policy_head_bench: no GPU")
    out = {"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "vf": list(ARCH[2]), "actions": ARCH[3]}}

    # (a) one PPO minibatch
    c = PC.make_inputs(ARCH, 512, "default", late=True, seed=9)
    head = m3l_amd.ActorCriticHead(ARCH[0], ARCH[3], net_arch=dict(pi=list(ARCH[1]), vf=list(ARCH[2])))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "actions", "old_log_prob", "advantages", "returns")}
    x = t["x"].clone().requires_grad_(True)

    def zero():
        x.grad = None
        for p in head.parameters():
            p.grad = None

    def hip(read):
        zero()
        loss, stats = head.ppo_loss(x, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], c["clip_range"], c["ent_coef"], c["vf_coef"])
        if read:
            stats.stats_dict()
        loss.backward()
        return loss

    def eager(read):
        zero()
        h = PC.head_forward(P, x, t["actions"])
        r = PC.ppo_loss_ref(h["values"], h["log_prob"], h["entropy"], t["old_log_prob"], t["advantages"], t["returns"], c["clip_range"], c["ent_coef"],
                            c["vf_coef"], sync=read)
        r["loss"].backward()
        return r["loss"]
    fns = {"hip": lambda: hip(False), "eager": lambda: eager(False), "hip_stats_read": lambda: hip(True), "eager_stats_read": lambda: eager(True)}
    res, last = alternate(fns, a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["loss"] = float(last[name].detach())
    res["hip"]["entry_points"] = entry_points(fns["hip"])
    res["hip_over_eager_call"] = round(res["hip"]["call_us"] / res["eager"]["call_us"], 3)
    res["hip_over_eager_call_stats_read"] = round(res["hip_stats_read"]["call_us"] / res["eager_stats_read"]["call_us"], 3)
    out["ppo_loss_fwd_bwd_B512"] = res

    # (b) one environment step
    xb = torch.randn(8, ARCH[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    noise = torch.randn(8, ARCH[3], generator=torch.Generator().manual_seed(4)).to(DEV)

    def hip_act():
        with torch.no_grad():
            return head(xb, noise=noise)

    def eager_act():
        with torch.no_grad():
            lat_pi, _ = PC._branch(P, "policy_net", xb)
            lat_vf, _ = PC._branch(P, "value_net", xb)
            mean = torch.nn.functional.linear(lat_pi, P["action_net.weight"], P["action_net.bias"])
            dist = torch.distributions.Normal(mean, torch.ones_like(mean) * P["log_std"].exp())
            actions = mean + P["log_std"].exp() * noise
            values = torch.nn.functional.linear(lat_vf, P["value_net.weight"], P["value_net.bias"]).flatten()
            return actions, values, dist.log_prob(actions).sum(dim=1)
    fns = {"hip": hip_act, "eager": eager_act}
    res, last = alternate(fns, 10 * a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["log_prob_sum"] = float(last[name][2].sum())
    res["hip"]["entry_points"] = entry_points(hip_act)
    res["hip_over_eager_call"] = round(res["hip"]["call_us"] / res["eager"]["call_us"], 3)
    out["act_no_grad_B8"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
