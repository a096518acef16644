"""The TD target with one discount per row on a real MI355X (m3l_sac_td_target_rows, `sac.td_target(gamma=tensor)`): what an n-step batch of
DeviceReplayBuffer feeds it, discounts = gamma^(steps walked).

Yardstick: the float64 restatement of tests/sac_cases.py (`step_ref`), whose target line broadcasts a (B, 1) gamma as it stands, under the SAC
head's bound (test_sac_head_gpu.py: 1e-4 max(1, |ref|)).  Shapes: the smallest legal widths — F = 16, one hidden layer of 16 per net, A = 1 and
3 — with B = 5 and 33, neither a multiple of the 16-row tile, 33 more than one workgroup.  The inputs are settled by sac_cases.make_inputs, so the
gates and the chosen critic are the same in float32 and float64; none of those conditions involves gamma."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import m3l_amd
import sac_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = 1e-4
CASES = [(5, 1), (5, 3), (33, 1), (33, 3)]


@lru_cache(maxsize=None)
def _case(B, A):
    c = SC.make_inputs((16, (16,), (16,), A), B, False, False, seed=4100 + 10 * B + A)
    g = np.random.default_rng(B + A)
    disc = (1.0 - g.random(B)).astype(np.float32)          # (0, 1]
    disc[0], disc[-1] = 1.0, np.float32(0.99) ** 3         # the edge of the range, and what a walk of three steps gives
    assert (disc > 0).all() and (disc <= 1).all()
    return c, disc


def _head(c):
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.SACHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)))
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}, strict=True)
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


@pytest.mark.parametrize("B,A", CASES)
def test_per_row_discounts_against_the_restatement(B, A):
    c, disc = _case(B, A)
    ref = SC.step_ref(dict(c, gamma=torch.from_numpy(disc.astype(np.float64)).reshape(B, 1)))["target_q"]
    head = _head(c)
    xn, r, d, noise = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next")
    dv = torch.from_numpy(disc).to(DEV)
    flat = head.td_target(xn, r, d, dv, ent_coef=c["ent_coef"], noise=noise)
    col = head.td_target(xn, r.reshape(B, 1), d.reshape(B, 1), dv.reshape(B, 1), ent_coef=c["ent_coef"], noise=noise)
    assert flat.shape == (B,) and flat.dtype == torch.float32 and not flat.requires_grad
    assert torch.equal(flat, col), "(B,) and (B, 1) discounts differ"
    assert torch.equal(flat, head.td_target(xn, r, d, dv, ent_coef=c["ent_coef"], noise=noise)), "two runs differ in their bits"
    got = flat.double().cpu().numpy()
    err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f"[td_target rows B={B} A={A}] err {err:.2e} (bound {VALUE_TOL:.0e})")
    assert err <= VALUE_TOL
    # the discounts matter: the scalar path with their mean is another vector, and a done row is its reward whatever the discount
    other = head.td_target(xn, r, d, float(disc.mean()), ent_coef=c["ent_coef"], noise=noise)
    assert not torch.equal(other, flat) and torch.equal(flat[1], r[1]) and float(d[1]) == 1.0
    # the pointer form of the entropy coefficient
    log_ent = torch.tensor([np.log(c["ent_coef"])], dtype=torch.float32, device=DEV)
    by_ptr = head.td_target(xn, r, d, dv, log_ent_coef=log_ent, noise=noise).double().cpu().numpy()
    assert float((np.abs(by_ptr - ref) / np.maximum(1.0, np.abs(ref))).max()) <= VALUE_TOL


@pytest.mark.parametrize("B,A", CASES)
def test_constant_discounts_give_the_bits_of_the_scalar_entry(B, A):
    c, _ = _case(B, A)
    head = _head(c)
    xn, r, d, noise = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next")
    for gamma in (0.99, 1.0, float(np.float32(0.99) ** 3), 0.5):
        scalar = head.td_target(xn, r, d, gamma, ent_coef=c["ent_coef"], noise=noise)
        rows = head.td_target(xn, r, d, torch.full((B, 1), gamma, dtype=torch.float32, device=DEV), ent_coef=c["ent_coef"], noise=noise)
        assert torch.equal(scalar, rows), gamma
    assert torch.equal(head.td_target(xn, r, d, np.float32(0.99), ent_coef=c["ent_coef"], noise=noise),
                       head.td_target(xn, r, d, float(np.float32(0.99)), ent_coef=c["ent_coef"], noise=noise))


def test_rejections():
    B, A = 5, 3
    c, disc = _case(B, A)
    head = _head(c)
    xn, r, d = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones")
    dv = torch.from_numpy(disc).to(DEV)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        head.td_target(xn, r, d, dv.cpu(), ent_coef=0.1)
    for bad in (dv[:-1], dv.repeat(2), dv.reshape(1, B), dv.double(), dv.to(torch.bfloat16), torch.ones(B, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="gamma: a number, or a float32 tensor of shape"):
            head.td_target(xn, r, d, bad, ent_coef=0.1)
    for bad in ("0.99", None, [0.99] * B, disc):
        with pytest.raises(ValueError, match="gamma: a number or a float32 CUDA tensor"):
            head.td_target(xn, r, d, bad, ent_coef=0.1)
