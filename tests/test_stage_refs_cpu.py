"""Anchors tests/stage_refs.py, the float64 yardstick of tests/test_stages_gpu.py.  CPU only.

  1. chained with the oracle's transformer, the stage functions give the loss and every gradient of oracle.vtmae_forward to 1e-12;
  2. fed with the tensors the reference's own run recorded (tests/golden/*.npz, `cap/*`), each stage reproduces the next recorded tensor;
  3. mask_sample reproduces the recorded argsort on tie-free rows and the stable argsort on every row;
  4. the `rnd` hook is live at every stage that stores something in the compute type, and is exactly the identity by default.
"""
import os

import numpy as np
import pytest
import torch

import stage_refs as R
from oracle import vtmae_oracle as O

CASES = ["vt_small", "vt_decdim", "v_only_small", "vt_learnedpos", "vt_cfg2_geom"]
F64 = torch.float64


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    cfg = O.cfg_from_meta(z["meta"], z["ratio"])
    sincos = bool(int(z["sincos"])) if "sincos" in z.files else True
    x = {k[len("input/"):]: torch.tensor(z[k]) for k in z.files if k.startswith("input/")}
    nn = len([k for k in z.files if k.startswith("noise/")])
    noises = [z[f"noise/{i}"] for i in range(nn)]
    perms = [z[f"argsort/{i}"] for i in range(nn)]
    return z, cfg, sincos, x, noises, perms


def _stage_args(P, cfg, sincos, x):
    """the stage functions' geometry, inputs and tensor groups for a fixture (what VTMAE._embed_tensors / _glue_tensors / _head_tensors build)"""
    k = cfg.num_tactiles
    g = R.make_geom(cfg.image_hw, cfg.image_patch, cfg.channels, cfg.tactile_hw, cfg.tactile_patch, cfg.channels, k, True, k > 0)
    n_img, N = cfg.n_img, cfg.n_total
    emb = [P.get(f"encoder.{m}_to_patch_embedding.{i}.{w}") for m in ("image", "tactile") for i in (1, 2, 3) for w in ("weight", "bias")]
    zero = lambda d: torch.zeros(1 + k, d, dtype=F64)
    if sincos:
        emb += [P["encoder_modality_embedding.weight"], P["image_enc_pos_embedding"][0], P["tactile_enc_pos_embedding"][0]]
        dpos = [P["decoder_modality_embedding.weight"], P["image_dec_pos_embedding"][0], P["tactile_dec_pos_embedding"][0]]
    else:
        pe, w = P["encoder.pos_embedding"][0], P["decoder_pos_emb.weight"]
        emb += [zero(cfg.dim), pe[1:1 + n_img], pe[1 + n_img:1 + N]]
        dpos = [zero(cfg.dec_dim), w[:n_img], w[n_img:N]]
    glue = [P.get("enc_to_dec.weight"), P.get("enc_to_dec.bias"), P["mask_token"]] + dpos
    heads = [P["to_pixels.weight"], P["to_pixels.bias"], P["to_tactiles.weight"], P["to_tactiles.bias"]]
    image = x["image"]
    tactiles = [x[f"tactile{i + 1}"] for i in range(k)]
    return g, image, tactiles, emb, glue, heads


@pytest.mark.parametrize("name", CASES)
def test_chain_equals_oracle(golden_dir, name):
    z, cfg, sincos, x, noises, _ = _load(golden_dir, name)
    P = O.load_fixture_params(z, dtype=F64, requires_grad=True)
    x64 = {k_: v.to(F64) for k_, v in x.items()}
    ref = O.vtmae_forward(P, cfg, x64, [torch.tensor(n) for n in noises], sincos=sincos)
    ref["loss"].backward()
    want = {k_: (None if v.grad is None else v.grad.clone()) for k_, v in P.items()}
    for v in P.values():
        v.grad = None

    g, image, tactiles, emb, glue, heads = _stage_args(P, cfg, sincos, x)
    masked, unmasked, c = R.mask_sample(g, cfg.ratio, noises)
    assert torch.equal(masked, ref["masked_indices"]) and torch.equal(unmasked, ref["unmasked_indices"])
    tokens = R.embed(g, cfg.dim, unmasked, c["n_img"] - c["nm_img"], c["num_unmasked"], image, tactiles, *emb)
    enc = O.transformer(tokens, P, "encoder.transformer.", cfg.depth, cfg.heads, cfg.dim_head)
    dec_in = R.unshuffle(g, cfg.dim, cfg.dec_dim, unmasked, masked, enc, enc, *glue)
    dec = O.transformer(dec_in, P, "decoder.", cfg.dec_depth, cfg.dec_heads, cfg.dec_dim_head)
    h = R.heads_loss(g, cfg.dec_dim, masked, c["nm_img"], image, tactiles, dec, *heads, dloss=1.0)
    dec.backward(h["d_dec"])
    for t, gr in zip(heads, h["grads"]):
        t.grad = gr

    tol = 1e-12
    assert abs(float(h["loss"]) - float(ref["loss"].detach())) <= tol * abs(float(ref["loss"].detach()))
    for key in ("encoder_in", "decoder_in", "pred_pixel", "target_pixel") + (("pred_tactile", "target_tactile") if cfg.num_tactiles else ()):
        mine = {"encoder_in": tokens, "decoder_in": dec_in}.get(key, h.get(key))
        assert float((mine - ref[key]).detach().abs().max()) <= tol * max(1.0, float(ref[key].detach().abs().max())), key
    checked = 0
    for key, w in want.items():
        got = P[key].grad
        if w is None:
            assert got is None or float(got.abs().max()) == 0.0, key
            continue
        assert got is not None, key
        assert float((got - w).abs().max()) <= tol * max(1.0, float(w.abs().max())), key
        checked += 1
    assert checked > 20


@pytest.mark.parametrize("name", CASES)
def test_stages_reproduce_the_recorded_run(golden_dir, name):
    """bound: 1e-5 absolute on tensors, 1e-6 relative on the loss (the float64 oracle sits <= 1.6e-6 / 1e-7 from these float32 captures)"""
    z, cfg, sincos, x, noises, perms = _load(golden_dir, name)
    P = O.load_fixture_params(z, dtype=F64)
    g, image, tactiles, emb, glue, heads = _stage_args(P, cfg, sincos, x)
    k = cfg.num_tactiles
    # the index lists of THIS reference run (its argsort is not stable on tied rows)
    m_np, u_np, nm_img, _ = O.mask_indices(noises, cfg.ratio, cfg.n_img, cfg.n_tac, k, perms)
    masked, unmasked = torch.from_numpy(m_np), torch.from_numpy(u_np)
    cap = lambda key: torch.tensor(z["cap/" + key]).to(F64)
    with torch.no_grad():
        tokens = R.embed(g, cfg.dim, unmasked, cfg.n_img - nm_img, unmasked.shape[1], image, tactiles, *emb)
        assert float((tokens - cap("encoder_in")).abs().max()) <= 1e-5
        allp = R.embed(g, cfg.dim, None, cfg.n_img, cfg.n_total, image, tactiles, *emb)       # all patches, then the gather
        assert float((R.gather_tokens(allp, unmasked) - tokens).abs().max()) <= 1e-13      # (BLAS blocks the two row counts differently)
        dec_in = R.unshuffle(g, cfg.dim, cfg.dec_dim, unmasked, masked, cap("encoder_out"), cap("encoder_out"), *glue)
        assert float((dec_in - cap("decoder_in")).abs().max()) <= 1e-5
        h = R.heads_loss(g, cfg.dec_dim, masked, nm_img, image, tactiles, cap("decoder_out"), *heads)
        assert abs(float(h["loss"]) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
        assert float((h["pred_pixel"] - cap("to_pixels_out")).abs().max()) <= 1e-5
        if k:
            assert float((h["pred_tactile"] - cap("to_tactiles_out")).abs().max()) <= 1e-5
        assert abs(float(h["loss_parts"].sum()) - float(h["loss"])) <= 1e-15


@pytest.mark.parametrize("name", CASES)
def test_mask_sample_against_recorded_argsort(golden_dir, name):
    z, cfg, sincos, x, noises, perms = _load(golden_dir, name)
    g = R.make_geom(cfg.image_hw, cfg.image_patch, cfg.channels, cfg.tactile_hw, cfg.tactile_patch, cfg.channels, cfg.num_tactiles, True,
                    cfg.num_tactiles > 0)
    masked, unmasked, c = R.mask_sample(g, cfg.ratio, noises)
    assert masked.dtype == torch.int64 and unmasked.dtype == torch.int64
    assert (c["nm_img"], c["nm_tac"]) == O.mask_counts(cfg.ratio, cfg.n_img, cfg.n_tac * cfg.num_tactiles, cfg.num_tactiles)[1:]
    assert c["num_masked"] == c["nm_img"] + cfg.num_tactiles * c["nm_tac"] and c["num_masked"] + c["num_unmasked"] == cfg.n_total
    # every row: numpy's stable argsort (the oracle's own code path) and torch's
    m_st, u_st, _, _ = O.mask_indices(noises, cfg.ratio, cfg.n_img, cfg.n_tac, cfg.num_tactiles)
    assert np.array_equal(masked.numpy(), m_st) and np.array_equal(unmasked.numpy(), u_st)
    for n in noises:
        assert np.array_equal(np.argsort(n, -1, kind="stable"), torch.tensor(n).argsort(dim=-1, stable=True).numpy())
    # tie-free noise rows: what the reference's run recorded, per modality segment of the two lists (some fixtures tie a row of
    # every sample in one modality or another, so whole samples are not always tie-free)
    m_rec, u_rec, _, _ = O.mask_indices(noises, cfg.ratio, cfg.n_img, cfg.n_tac, cfg.num_tactiles, perms)
    m0 = u0 = seen = 0
    for i, n in enumerate(noises):
        nm = c["nm_img"] if i == 0 else c["nm_tac"]
        free = np.array([len(np.unique(n[r])) == n.shape[1] for r in range(n.shape[0])])
        seen += int(free.sum())
        assert np.array_equal(masked.numpy()[free, m0:m0 + nm], m_rec[free, m0:m0 + nm])
        assert np.array_equal(unmasked.numpy()[free, u0:u0 + n.shape[1] - nm], u_rec[free, u0:u0 + n.shape[1] - nm])
        m0, u0 = m0 + nm, u0 + n.shape[1] - nm
    assert seen > 0 and m0 == masked.shape[1] and u0 == unmasked.shape[1]
    # explicit counts (VTMAE.reconstruct's rule), the two extremes included
    for cnt in ((0, 0), (cfg.n_img, cfg.n_tac if cfg.num_tactiles else 0), (3, 1 if cfg.num_tactiles else 0)):
        m2, u2, c2 = R.mask_sample(g, cfg.ratio, noises, counts=cnt)
        m3, u3, _, _ = O.mask_indices(noises, cfg.ratio, cfg.n_img, cfg.n_tac, cfg.num_tactiles, counts=cnt)
        assert np.array_equal(m2.numpy(), m3) and np.array_equal(u2.numpy(), u3)
        assert m2.shape[1] == c2["num_masked"] and u2.shape[1] == c2["num_unmasked"]


def _rand_case(seed=0):
    """a small two-modality case with enc_to_dec, parameters away from initialisation"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    k, D, dd = 2, 32, 16
    g = R.make_geom(16, 4, 3, 8, 4, 3, k)
    n_img, n_tac, _ = R.geo(g)
    N = n_img + k * n_tac
    pd = 48
    grp = lambda: [1 + 0.5 * rn(pd), 0.4 * rn(pd), 2 / pd ** 0.5 * rn(D, pd), 0.4 * rn(D), 1 + 0.5 * rn(D), 0.4 * rn(D)]
    emb = grp() + grp() + [0.4 * rn(1 + k, D), rn(n_img, D), rn(k * n_tac, D)]
    glue = [2 / D ** 0.5 * rn(dd, D), 0.4 * rn(dd), 0.4 * rn(dd), 0.4 * rn(1 + k, dd), rn(n_img, dd), rn(k * n_tac, dd)]
    heads = [2 / dd ** 0.5 * rn(pd, dd), 0.4 * rn(pd), 2 / dd ** 0.5 * rn(pd, dd), 0.4 * rn(pd)]
    for t in emb + glue:
        t.requires_grad_(True)
    B = 3
    image = torch.rand(B, 3, 16, 16, generator=gen)
    tactiles = [torch.rand(B, 3, 8, 8, generator=gen) for _ in range(k)]
    noises = [torch.rand(B, n, generator=gen).numpy() for n in [n_img] + [n_tac] * k]
    masked, unmasked, c = R.mask_sample(g, 0.75, noises)
    return g, D, dd, emb, glue, heads, image, tactiles, masked, unmasked, c, rn, B, N


def _stage_results(rnd_kw):
    g, D, dd, emb, glue, heads, image, tactiles, masked, unmasked, c, rn, B, N = _rand_case()
    out = {}
    tok = R.embed(g, D, unmasked, c["n_img"] - c["nm_img"], c["num_unmasked"], image, tactiles, *emb, **rnd_kw)
    out["embed"] = [tok] + R.grads_of(tok, rn(*tok.shape), emb)
    enc = R.bf16_rnd(rn(B, c["num_unmasked"], D)).requires_grad_(True)
    di = R.unshuffle(g, D, dd, unmasked, masked, enc, enc, *glue, **rnd_kw)
    out["unshuffle"] = [di] + R.grads_of(di, rn(*di.shape), [enc] + glue)
    h = R.heads_loss(g, dd, masked, c["nm_img"], image, tactiles, R.bf16_rnd(rn(B, N, dd)), *heads, dloss=0.37, **rnd_kw)
    out["heads"] = [h["loss"], h["d_dec"], h["pred_pixel"], h["pred_tactile"]] + h["grads"]
    return out


def test_rnd_hook_is_live_and_identity_by_default():
    exact, same, emu = _stage_results({}), _stage_results(dict(rnd=lambda t: t)), _stage_results(dict(rnd=R.bf16_rnd))
    for stage in exact:
        for a, b in zip(exact[stage], same[stage]):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(a, b), stage
    # embed: tokens and every parameter gradient of both groups move; the second LayerNorm's bias and the modality rows are sums of the
    # f32 cotangent (downstream of no rounding) and stay exact in the backward only through dE's consumers — they read dtokens, not dE
    e, m = exact["embed"], emu["embed"]
    moved = [not torch.equal(a, b) for a, b in zip(e, m) if a is not None]
    assert moved[0] and all(moved[1 + i] for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)), moved
    assert torch.equal(e[1 + 5], m[1 + 5]) and torch.equal(e[1 + 11], m[1 + 11]) and torch.equal(e[1 + 12], m[1 + 12])
    assert torch.equal(e[1 + 13], m[1 + 13]) and torch.equal(e[1 + 14], m[1 + 14])
    # unshuffle: dec_in, d_enc and dW move; the bias, mask-token, modality and position gradients do not
    e, m = exact["unshuffle"], emu["unshuffle"]
    assert not torch.equal(e[0], m[0]) and not torch.equal(e[1], m[1]) and not torch.equal(e[2], m[2])
    for i in (3, 4, 5, 6, 7):
        assert torch.equal(e[i], m[i]), i
    # heads: everything moves
    for a, b in zip(exact["heads"], emu["heads"]):
        assert not torch.equal(a, b)
    # ... by no more than a few bf16 roundings (2^-8 relative each)
    for stage in exact:
        for a, b in zip(exact[stage], emu[stage]):
            if a is not None:
                assert float((a - b).detach().abs().max()) <= 0.05 * float(a.detach().abs().max()), stage


def test_heads_gradients_are_the_autograd_ones():
    """heads_loss writes its backward out by hand: with rnd the identity it is d(dloss * loss) by autograd"""
    g, D, dd, emb, glue, heads, image, tactiles, masked, unmasked, c, rn, B, N = _rand_case(1)
    dec = rn(B, N, dd).requires_grad_(True)
    hw = [t.clone().requires_grad_(True) for t in heads]
    pi, pt = R.patches_of(g, image, tactiles)
    br = torch.arange(B)[:, None]
    mi, mt = masked[:, :c["nm_img"]], masked[:, c["nm_img"]:]
    loss = torch.nn.functional.mse_loss(dec[br, mi] @ hw[0].t() + hw[1], pi[br, mi]) \
        + 10 * torch.nn.functional.mse_loss(dec[br, mt] @ hw[2].t() + hw[3], pt[br, mt - c["n_img"]])
    want = torch.autograd.grad(loss * 0.37, [dec] + hw)
    h = R.heads_loss(g, dd, masked, c["nm_img"], image, tactiles, dec, *heads, dloss=0.37)
    assert abs(float(h["loss"] - loss.detach())) <= 1e-14 * abs(float(loss.detach()))
    for a, b in zip([h["d_dec"]] + h["grads"], want):
        assert float((a - b).abs().max()) <= 1e-14 * max(1.0, float(b.abs().max()))
    vis = torch.ones(B, N, dtype=torch.bool)
    vis[br, masked] = False
    assert float(h["d_dec"][vis].abs().max()) == 0.0


def test_tokens_assemble_and_scatter():
    g, D, dd, emb, glue, heads, image, tactiles, masked, unmasked, c, rn, B, N = _rand_case(2)
    n_img, n_tac, k = R.geo(g)
    img_tok, tac = rn(B, n_img, D), rn(B, k, n_tac, D)
    tok = R.tokens_assemble(g, D, img_tok, tac.permute(1, 0, 2, 3).reshape(k * B, n_tac, D), *emb[12:])
    want = torch.cat([img_tok + emb[12][0] + emb[13], tac.reshape(B, k * n_tac, D) + emb[12][1:].repeat_interleave(n_tac, 0) + emb[14]], 1)
    assert torch.equal(tok, want)
    x = rn(B, N, D)
    y = R.gather_tokens(x, unmasked)
    back = R.scatter_tokens(y, unmasked, N)
    assert torch.equal(back[torch.arange(B)[:, None], unmasked], y) and float(back[torch.arange(B)[:, None], masked].abs().max()) == 0.0
