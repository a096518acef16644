"""What the policy heads (policy.py: PPO, Tanh, "branch"; sac.py and the heads built on it, sac_ensemble.py, tqc.py, td3.py: ReLU, "net") do alike
on the Python side: reading Linear / activation pairs out of a module, walking a net's layer shapes, the limits of the kernels
(csrc/policy_common.cuh), and preparing features, noise, actions, weights and row vectors for a call.  Every function takes what differs as an
argument: the activation class, and the head's name (`head`: "policy" / "SAC" / "TD3") and its word for one net (`noun`) for the messages.
Only `scale_coef`, the backward that the critic heads' losses share, launches a kernel."""
import numbers

import torch
from torch import nn

from . import _lib as L
from .functional import _require_cuda, _stream

MAX_HIDDEN, MAX_WIDTH, MAX_ACTIONS = 3, 512, 64


def mlp(k, widths, act, out=None):
    """nn.Sequential of Linear at the even and `act` at the odd indices over an input of width k, then Linear(., out) when `out` is given."""
    mods = []
    for w in widths:
        mods += [nn.Linear(k, w), act()]
        k = w
    if out is not None:
        mods.append(nn.Linear(k, out))
    return nn.Sequential(*mods)


def linear_pairs(seq, name, act, head):
    """((weight, bias), ...) of the Linears of `seq`, which must be Linear / `act` pairs."""
    mods = list(seq)
    if len(mods) % 2:
        raise ValueError(f"{name}: Linear / {act.__name__} pairs expected, got {len(mods)} modules")
    out = []
    for i in range(0, len(mods), 2):
        if not isinstance(mods[i], nn.Linear) or mods[i].bias is None:
            raise ValueError(f"{name}.{i}: nn.Linear with a bias expected, got {type(mods[i]).__name__}")
        if not isinstance(mods[i + 1], act):
            raise ValueError(f"{name}.{i + 1}: the HIP {head} head computes {act.__name__} only, got {type(mods[i + 1]).__name__}")
        out.append((mods[i].weight, mods[i].bias))
    return tuple(out)


def layer_widths(k, layers, name, head, noun):
    """(width of the last layer, (widths)) of the hidden `layers` ((weight, bias), ...) of one net over an input of width k; their count and
    every shape checked."""
    if len(layers) > MAX_HIDDEN:
        raise ValueError(f"{name}: {len(layers)} hidden layers (the HIP {head} head runs 0 to {MAX_HIDDEN} per {noun})")
    ws = []
    for l, (w, b) in enumerate(layers):
        if w.dim() != 2 or w.shape[1] != k or tuple(b.shape) != (w.shape[0],):
            raise ValueError(f"{name} layer {l}: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not follow an input of width {k}")
        k = int(w.shape[0])
        ws.append(k)
    return k, tuple(ws)


def check_head_linear(name, wb, n, k):
    w, b = wb
    if tuple(w.shape) != (n, k) or tuple(b.shape) != (n,):
        raise ValueError(f"{name}: weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected ({n}, {k}) / ({n},)")


def check_widths(widths, first="features"):
    for w in widths:
        if w < 16 or w % 16 or w > MAX_WIDTH:
            raise ValueError(f"width {w}: {first} and hidden widths must be multiples of 16, at most {MAX_WIDTH}")


def check_limits(widths, A):
    """The kernels' limits on the features' and hidden widths and on the action count of a head given by its tensors."""
    check_widths(widths)
    if not 1 <= A <= MAX_ACTIONS:
        raise ValueError(f"{A} action dimensions (1 to {MAX_ACTIONS})")


def check_float32(flat, head):
    for t in flat:
        if t.dtype != torch.float32:
            raise ValueError(f"{head} head parameter of dtype {t.dtype}: the HIP {head} head computes in float32 and returns float32 gradients; "
                             "keep the head's parameters in float32 whatever the encoder's compute type")


def require_params(flat, what):
    for t in flat:
        _require_cuda(t, what)


def action_dim_of(action_dim, head):
    """The `action_dim` argument of a head class as an int; an action space or anything else that is no integer is refused."""
    if hasattr(action_dim, "n") or hasattr(action_dim, "nvec"):
        raise ValueError(f"action_dim={action_dim!r}: discrete action spaces are not computed by the HIP {head} head; pass the length of a "
                         "continuous (Box) action vector")
    if isinstance(action_dim, bool) or not isinstance(action_dim, numbers.Integral):
        raise ValueError(f"action_dim={action_dim!r}: an integer expected, the length of a continuous (Box) action vector")
    return int(action_dim)


def head_dims(features_dim, action_dim, net_arch, default, other, head, noun, first="features"):
    """The constructor arguments of a head class -> (features_dim, action_dim, pi widths, `other` widths) inside the kernels' limits.  net_arch:
    dict(pi=[...], <other>=[...]), one list for both, or None for `default` widths in both."""
    action_dim = action_dim_of(action_dim, head)
    if net_arch is None:
        net_arch = default
    if isinstance(net_arch, (list, tuple)):
        net_arch = {"pi": list(net_arch), other: list(net_arch)}
    pi, ot = [int(w) for w in net_arch.get("pi", [])], [int(w) for w in net_arch.get(other, [])]
    check_widths([int(features_dim)] + pi + ot, first)
    if len(pi) > MAX_HIDDEN or len(ot) > MAX_HIDDEN:
        raise ValueError(f"net_arch {net_arch}: 0 to {MAX_HIDDEN} hidden layers per {noun}")
    if not 1 <= action_dim <= MAX_ACTIONS:
        raise ValueError(f"action_dim={action_dim}: 1 to {MAX_ACTIONS}")
    return int(features_dim), action_dim, pi, ot


def _dev(t):
    """float32, contiguous, 16-byte aligned, detached."""
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.contiguous().float()
    return t.clone() if t.data_ptr() % 16 else t


def _rows(x, what, width=None):
    _require_cuda(x, what)
    if x.dim() != 2 or x.shape[0] < 1 or (width is not None and x.shape[1] != width):
        raise ValueError(f"{what}: (B, {width if width is not None else 'F'}) expected, got {tuple(x.shape)}")
    return _dev(x)


def _vec(t, what, B):
    _require_cuda(t, what)
    if t.numel() != B:
        raise ValueError(f"{what}: {B} values expected, got {tuple(t.shape)}")
    return _dev(t).reshape(B)


def features_of(features, on_tape):
    """features (B, F) as the kernels read them: float32, contiguous, 16-byte aligned.  on_tape: by differentiable operations, so that the
    features take the gradient; else detached."""
    _require_cuda(features, "features")
    if features.dim() != 2 or features.shape[0] < 1:
        raise ValueError(f"features: (B, F) expected, got {tuple(features.shape)}")
    if not on_tape:
        return _dev(features)
    x = features.float().contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def noise_of(noise, B, A, device, deterministic=False):
    """The standard-normal draw (B, A) of a call: none when deterministic, torch.randn when not given."""
    if deterministic:
        return None
    if noise is None:
        return torch.randn(B, A, dtype=torch.float32, device=device)
    noise = _rows(noise, "noise", A)
    if noise.shape[0] != B:
        raise ValueError(f"{B} feature rows but {noise.shape[0]} noise rows")
    return noise


def actions_of(actions, B, A):
    """actions (B, A) beside B feature rows as the critics read them: float32, contiguous, 16-byte aligned, by differentiable operations."""
    _require_cuda(actions, "actions")
    if actions.dim() != 2 or actions.shape[1] != A:
        raise ValueError(f"actions: (B, {A}) expected, got {tuple(actions.shape)}")
    if actions.shape[0] != B:
        raise ValueError(f"{B} feature rows but {actions.shape[0]} action rows")
    a = actions.float().contiguous()
    return a.clone() if a.data_ptr() % 16 else a


def weights_of(weights, B):
    """The importance weights of a critic loss, float32 (B,) or (B, 1), as the kernels read them; None (ones) stays None."""
    if weights is None:
        return None
    _require_cuda(weights, "weights")
    if weights.dtype != torch.float32 or tuple(weights.shape) not in ((B,), (B, 1)):
        raise ValueError(f"weights: a float32 tensor of shape ({B},) or ({B}, 1) expected, got {tuple(weights.shape)} {weights.dtype}")
    return _vec(weights, "weights", B)


def scale_coef(dloss, coef):
    """The backward of a loss whose forward stored coef = d loss / d input: dloss * coef in coef's shape, one launch (m3l_sac_ens_loss_bwd)."""
    out = torch.empty_like(coef)
    L.check(L.lib().m3l_sac_ens_loss_bwd(L.ptr(_dev(dloss)), L.ptr(coef), coef.numel(), L.ptr(out), _stream()), "m3l_sac_ens_loss_bwd")
    return out


def require_shared_extractor(module, head, name=None):
    """Refuses a policy or critic module with share_features_extractor=False; name: the sub-module's, in front of the message."""
    if not getattr(module, "share_features_extractor", True):
        raise ValueError(f"{name + ': ' if name else ''}share_features_extractor=False: the HIP {head} head takes one feature vector for the actor and "
                         "the critics")


def no_workspace(node):
    return L.M3LError(f"{node}: the forward ran without a workspace (store=False), so it has no backward")
