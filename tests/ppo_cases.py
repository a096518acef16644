"""Float64 restatement of the PPO policy head and loss, and the inputs of its tests (test_policy_head_cpu.py, test_policy_head_gpu.py,
golden/make_golden_ppo_head.py, tools/policy_head_bench.py).

The head — Stable-Baselines3's ActorCriticPolicy behind its features extractor, with `net_arch = dict(pi=[...], vf=[...])` and Tanh as the
reference configures it (train.py:166) — is built from torch primitives (nn.functional.linear, torch.tanh, torch.distributions.Normal,
autograd).  SB3 is not part of the reference tree, so that part is a restatement of SB3 2.x's MlpExtractor, DiagGaussianDistribution and
ActorCriticPolicy.evaluate_actions: PARITY UNPINNED.  The loss follows models/ppo_mae.py line by line, and test_policy_head_cpu.py pins it to
results recorded from the reference's own `PPO_MAE.train` (golden/ppo_head_step.npz).

Inputs are trained-like, not initialisation statistics: the weights of every hidden layer are scaled until its pre-activations have a standard
deviation of 1.6 (about a fifth of the units beyond |pre| = 2, where tanh' < 0.07), actions lie within two standard deviations of the mean, and
the "late-epoch" cases take old_log_prob from perturbed parameters so that a share of the rows between 0.2 and 0.8 is clipped."""
import math
from functools import lru_cache

import numpy as np
import torch
from torch.nn import functional as F

PRE_STD = 1.6
MARGIN = 1e-3               # no ratio this close to 1 +- clip_range, no |v - v_old| this close to clip_range_vf
CLIP_RANGE = 0.2
CLIP_RANGE_VF = 0.3

# (features, pi widths, vf widths, actions)
ARCHS = {
    "a64": (64, (64, 64), (64, 64), 3),
    "a256": (256, (256, 256), (256, 256), 7),
    "mixed": (32, (32,), (64, 48, 16), 1),
    "nopi": (48, (), (16,), 2),
    "golden": (32, (32, 32), (32, 32), 3),
    "novf": (16, (16,), (), 1),
    "plain": (16, (), (), 2),
}
# flag combinations of the loss: name -> (clip_range_vf, normalize_advantage)
FLAGS = {"default": (None, True), "vfclip": (CLIP_RANGE_VF, True), "nonorm": (None, False)}
ENT_COEF, VF_COEF = 0.01, 0.5

# name -> (arch, B, flags, late); late-epoch cases have at least 15 rows, so that a share of clipped rows between 0.2 and 0.8 can be asked of them
GPU_CASES = {
    "a64_b1": ("a64", 1, "default", False),
    "a64_b2": ("a64", 2, "vfclip", False),
    "a64_b3": ("a64", 3, "nonorm", False),
    "a64_b15": ("a64", 15, "default", True),
    "a64_b17": ("a64", 17, "vfclip", True),
    "a64_b33": ("a64", 33, "nonorm", True),
    "a64_b63": ("a64", 63, "vfclip", True),
    "a64_b65": ("a64", 65, "default", True),
    "a64_b130": ("a64", 130, "vfclip", True),
    "a256_b17": ("a256", 17, "default", True),
    "a256_b130": ("a256", 130, "vfclip", True),
    "mixed_b15": ("mixed", 15, "vfclip", True),
    "mixed_b33": ("mixed", 33, "nonorm", True),
    "mixed_b65": ("mixed", 65, "default", True),
    "nopi_b3": ("nopi", 3, "default", False),
    "nopi_b63": ("nopi", 63, "vfclip", True),
    "nopi_b130": ("nopi", 130, "nonorm", True),
    "novf_b3": ("novf", 3, "default", False),
    "novf_b17": ("novf", 17, "vfclip", True),
    "plain_b2": ("plain", 2, "vfclip", False),
    "plain_b33": ("plain", 33, "default", True),
}


def param_names(arch):
    """State-dict names of a head in SB3's layout, in the order of HeadParams.flat (pi, vf, action_net, value_net, log_std)."""
    _, pi, vf, _ = arch
    names = []
    for br, n in (("policy_net", len(pi)), ("value_net", len(vf))):
        for l in range(n):
            names += [f"mlp_extractor.{br}.{2 * l}.weight", f"mlp_extractor.{br}.{2 * l}.bias"]
    return names + ["action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std"]


def _branch(P, br, x):
    """SB3 MlpExtractor branch: Linear, Tanh, Linear, Tanh, ...; also every pre-activation."""
    pres, l = [], 0
    while f"mlp_extractor.{br}.{2 * l}.weight" in P:
        pre = F.linear(x, P[f"mlp_extractor.{br}.{2 * l}.weight"], P[f"mlp_extractor.{br}.{2 * l}.bias"])
        pres.append(pre)
        x = torch.tanh(pre)
        l += 1
    return x, pres


def head_forward(P, x, actions):
    """SB3 ActorCriticPolicy.evaluate_actions after extract_features, DiagGaussianDistribution: values (B,), log_prob (B,), entropy (B,), and
    the mean actions and pre-activations for the input checks.  What ppo_mae.py:280-281 receives (values already flat)."""
    latent_pi, pre_pi = _branch(P, "policy_net", x)
    latent_vf, pre_vf = _branch(P, "value_net", x)
    mean = F.linear(latent_pi, P["action_net.weight"], P["action_net.bias"])
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * P["log_std"].exp())
    log_prob = dist.log_prob(actions).sum(dim=1)
    entropy = dist.entropy().sum(dim=1)
    values = F.linear(latent_vf, P["value_net.weight"], P["value_net.bias"]).flatten()
    return dict(values=values, log_prob=log_prob, entropy=entropy, mean=mean, pre=pre_pi + pre_vf)


def closed_forms(mean, log_std, actions):
    """The header's formulas for log_prob and entropy."""
    lp = (-(actions - mean) ** 2 / (2 * torch.exp(2 * log_std)) - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    en = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum(-1).expand(mean.shape[0])
    return lp, en


def ppo_loss_ref(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, clip_range_vf=None, old_values=None,
                 normalize_advantage=True, sync=False):
    """models/ppo_mae.py:283-331 on tensors of any float dtype -> dict(loss, the five statistics, ratio, clipped count), all tensors.  sync: also
    read the logged values to the host where the reference does (`.item()` at :297, :298, :312, :321, `.cpu().numpy()` at :331); the tools time that."""
    if normalize_advantage and len(advantages) > 1:                                             # :285-286
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)                                                  # :289
    policy_loss_1 = advantages * ratio                                                          # :292
    policy_loss_2 = advantages * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)             # :293
    policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()                               # :294
    clipped = (torch.abs(ratio - 1) > clip_range)                                               # :298
    clip_fraction = torch.mean(clipped.float())
    if sync:
        policy_loss.item(), clip_fraction.item()                                                # :297-298
    if clip_range_vf is None:                                                                   # :301-309
        values_pred = values
    else:
        values_pred = old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = F.mse_loss(returns, values_pred)                                               # :311
    if sync:
        value_loss.item()                                                                       # :312
    entropy_loss = -torch.mean(entropy)                                                         # :319
    if sync:
        entropy_loss.item()                                                                     # :321
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss                         # :323
    with torch.no_grad():                                                                       # :329-331
        log_ratio = log_prob - old_log_prob
        approx_kl = torch.mean((torch.exp(log_ratio) - 1) - log_ratio)
        if sync:
            approx_kl.cpu().numpy()
    return dict(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, clip_count=clipped.sum(), clip_fraction=clip_fraction,
                approx_kl=approx_kl, ratio=ratio.detach())


STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl")


def make_params(arch, seed):
    """{name: float32 numpy array}: trained-like parameters of a head (see the module docstring)."""
    Fd, pi, vf, A = arch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rn(512, Fd)
    P = {}
    for br, widths in (("policy_net", pi), ("value_net", vf)):
        h = x
        for l, w in enumerate(widths):
            W, b = rn(w, h.shape[1]), 0.2 * rn(w)
            W = W * (PRE_STD / float(F.linear(h, W).std()))
            P[f"mlp_extractor.{br}.{2 * l}.weight"], P[f"mlp_extractor.{br}.{2 * l}.bias"] = W, b
            h = torch.tanh(F.linear(h, W, b))
        hn = A if br == "policy_net" else 1
        W = rn(hn, h.shape[1])
        W = W * ((0.8 if br == "policy_net" else 2.0) / float(F.linear(h, W).std()))
        name = "action_net" if br == "policy_net" else "value_net"
        P[name + ".weight"], P[name + ".bias"] = W, 0.1 * rn(hn)
    P["log_std"] = -0.7 + 0.8 * torch.rand(A, generator=g, dtype=torch.float64)
    return {k: P[k].float().numpy() for k in param_names(arch)}


def as_torch(P, dtype=torch.float64, device="cpu", requires_grad=False):
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype).requires_grad_(requires_grad) for k, v in P.items()}


def make_inputs(arch, B, flags, late, seed):
    """One minibatch for a head: parameters, features, actions within 2 sigma of the mean, advantages, returns, old values, old log-probabilities
    (late: from perturbed parameters, so that rows are clipped; else close to the current ones) and the loss flags.  float32 numpy arrays."""
    Fd, pi, vf, A = arch
    clip_range_vf, normalize = FLAGS[flags]
    P = make_params(arch, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, Fd, generator=g, dtype=torch.float64).float().double()
    P64 = as_torch(P)
    with torch.no_grad():
        mean = head_forward(P64, x, torch.zeros(B, A, dtype=torch.float64))["mean"]
        u = 4.0 * torch.rand(B, A, generator=g, dtype=torch.float64) - 2.0
        actions = (mean + P64["log_std"].exp() * u).float().double()
        cur = head_forward(P64, x, actions)
        # the parameters of an earlier epoch: action_net and log_std a little away
        scale = 0.35 if late else 0.02
        Q = dict(P64)
        Q["action_net.bias"] = P64["action_net.bias"] + scale * 0.5 * torch.randn(A, generator=g, dtype=torch.float64) / math.sqrt(A)
        Q["log_std"] = P64["log_std"] + scale * 0.3 * torch.randn(A, generator=g, dtype=torch.float64) / math.sqrt(A)
        old_log_prob = head_forward(Q, x, actions)["log_prob"].float().double()
        old_log_prob += scale * 0.6 * torch.randn(B, generator=g, dtype=torch.float64)
        old_log_prob = old_log_prob.float().double()
        advantages = (0.3 + 1.5 * torch.randn(B, generator=g, dtype=torch.float64)).float().double()
        returns = (cur["values"] + 0.8 * torch.randn(B, generator=g, dtype=torch.float64)).float().double()
        old_values = (cur["values"] + 0.35 * torch.randn(B, generator=g, dtype=torch.float64)).float().double()
        # keep every row away from the two clipping edges: these are inputs, moved by a step well above the margin
        for _ in range(20):
            r = torch.exp(cur["log_prob"] - old_log_prob)
            near = ((r - (1 - CLIP_RANGE)).abs() < 4 * MARGIN) | ((r - (1 + CLIP_RANGE)).abs() < 4 * MARGIN)
            if not bool(near.any()):
                break
            old_log_prob = (old_log_prob - 0.02 * near.double()).float().double()
        for _ in range(20):
            near = ((cur["values"] - old_values).abs() - CLIP_RANGE_VF).abs() < 4 * MARGIN
            if not bool(near.any()):
                break
            old_values = (old_values + 0.02 * near.double()).float().double()
    f32 = lambda t: t.float().numpy()      # noqa: E731
    return dict(params=P, x=f32(x), actions=f32(actions), old_log_prob=f32(old_log_prob), advantages=f32(advantages), returns=f32(returns),
                old_values=f32(old_values), clip_range=CLIP_RANGE, clip_range_vf=clip_range_vf, normalize_advantage=normalize, ent_coef=ENT_COEF,
                vf_coef=VF_COEF, arch=arch, late=late)


@lru_cache(maxsize=None)
def gpu_case(name):
    arch, B, flags, late = GPU_CASES[name]
    return make_inputs(ARCHS[arch], B, flags, late, seed=1000 + sorted(GPU_CASES).index(name))


def run_ref(c, dtype=torch.float64, device="cpu", dloss=1.0):
    """The restatement on a case in `dtype`: values, log_prob, entropy, loss, the statistics, the gradient of dloss * loss in the features and every
    parameter, as float64 numpy (clip_count: int)."""
    P = as_torch(c["params"], dtype, device, requires_grad=True)
    t = lambda k: torch.from_numpy(c[k]).to(device=device, dtype=dtype)      # noqa: E731
    x = t("x").requires_grad_(True)
    h = head_forward(P, x, t("actions"))
    r = ppo_loss_ref(h["values"], h["log_prob"], h["entropy"], t("old_log_prob"), t("advantages"), t("returns"), c["clip_range"], c["ent_coef"],
                     c["vf_coef"], c["clip_range_vf"], t("old_values") if c["clip_range_vf"] is not None else None, c["normalize_advantage"])
    (dloss * r["loss"]).backward()
    n64 = lambda v: v.detach().double().cpu().numpy()      # noqa: E731
    out = dict(values=n64(h["values"]), log_prob=n64(h["log_prob"]), entropy=n64(h["entropy"]), mean=n64(h["mean"]), loss=float(r["loss"].detach()),
               clip_count=int(r["clip_count"]), ratio=n64(r["ratio"]), pre=[n64(p) for p in h["pre"]])
    for k in STAT_NAMES:
        out[k] = float(r[k].detach())
    out["clip_fraction"] = out["clip_count"] / len(out["ratio"])          # exact: the reference's own figure is the float32 mean of a 0 / 1 mask
    out["grad"] = {"x": n64(x.grad)}
    for k, p in P.items():
        out["grad"][k] = n64(p.grad) if p.grad is not None else np.zeros(tuple(p.shape))
    return out


@lru_cache(maxsize=None)
def gpu_reference(name):
    return run_ref(gpu_case(name))


def eval_ref(c, dvalues, dlogp, dentropy, dtype=torch.float64):
    """evaluate_actions alone with given output gradients: outputs and the gradients in the features and parameters."""
    P = as_torch(c["params"], dtype, requires_grad=True)
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_(True)
    h = head_forward(P, x, torch.from_numpy(c["actions"]).to(dtype))
    s = (h["values"] * torch.from_numpy(dvalues).to(dtype)).sum() + (h["log_prob"] * torch.from_numpy(dlogp).to(dtype)).sum() + \
        (h["entropy"] * torch.from_numpy(dentropy).to(dtype)).sum()
    s.backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {"x": n64(x.grad)}
    grad.update({k: n64(p.grad) for k, p in P.items()})
    return dict(values=n64(h["values"]), log_prob=n64(h["log_prob"]), entropy=n64(h["entropy"]), grad=grad)


def conditions(c, ref):
    """What the GPU comparisons rest on, from the float64 run: distance of the ratios from the clipping edges, of |v - v_old| from clip_range_vf,
    the clipped share, and the share of hidden units with |pre| > 2."""
    r = ref["ratio"]
    ratio_gap = float(np.minimum(np.abs(r - (1 - c["clip_range"])), np.abs(r - (1 + c["clip_range"]))).min())
    v_gap = float(np.abs(np.abs(ref["values"] - c["old_values"].astype(np.float64)) - CLIP_RANGE_VF).min())
    pre = np.concatenate([p.ravel() for p in ref["pre"]]) if ref["pre"] else np.zeros(0)
    return dict(ratio_gap=ratio_gap, v_gap=v_gap, clipped_share=ref["clip_count"] / len(r),
                saturated=float((np.abs(pre) > 2).mean()) if pre.size else None,
                action_sigmas=float(np.abs((c["actions"] - ref["mean"]) / np.exp(c["params"]["log_std"].astype(np.float64))).max()))
