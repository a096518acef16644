"""The memory contract (tests/memguard.py, test_memory_contract_gpu.py) for the entry points of n-step returns: m3l_replay_nstep_rows,
m3l_replay_gather_load_rows2, m3l_replay_gather_load_frames_rows2 and m3l_sac_td_target_rows write nothing outside the outputs they were
handed and read nothing that nobody wrote.  Every output of theirs is allocated inside m3l_amd, so inside a MemGuard it lies between two
guards and is pre-filled with 0xFF (NaN) or 0x00: equal bits across the fills and intact guards.

Shapes: the smallest of test_replay_nstep_gpu.py — T = 7 steps of 2 environments, frame stacks 1, 2 and 4, the vector and the element-wise
paths, uint8 and float32 stores — with n_steps = 3 on a full ring with pos = 3, where the walks from steps 5 and 6 wrap the ring end; every
row of the ring is sampled, and B = 14 rows of the smallest image (25 pixels) is less than one workgroup, of the largest more than one."""
import numpy as np
import pytest
import torch

import memguard as MG
import nstep_cases as NC
import sac_cases as SC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402

DEV = "cuda:0"
T, E, A = NC.T, NC.E, NC.A
U8, F32 = np.uint8, np.float32
N, GAMMA = 3, 0.97


def _filled(fs, image_hw, tactile_hw, S, dtypes, frame_dedup, seed):
    st = NC.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=seed)
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    buf = m3l_amd.DeviceReplayBuffer(T * E, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, frame_dedup=frame_dedup, n_steps=N, gamma=GAMMA,
                                     device=DEV)
    for k in range(17):
        buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
                st["dones"][k], st["infos"][k])
    return buf


def test_memory_contract_of_the_nstep_entry_points(monkeypatch):
    cases = [(fs, (8, 8), (4, 4), 1, (U8, F32)) for fs in (1, 2, 4)] + [(2, (5, 5), (5, 3), 3, (F32, U8)), (4, (5, 5), (4, 4), 2, (F32, F32))]
    made = [(fs, _filled(fs, ihw, thw, S, dt, False, 500 + i), _filled(fs, ihw, thw, S, dt, True, 500 + i)) for i, (fs, ihw, thw, S, dt) in enumerate(cases)]
    every = torch.arange(T * E, dtype=torch.int64, device=DEV)
    env = NC.RewardNorm()

    def work(g):
        out = {}
        for i, (fs, sbuf, dbuf) in enumerate(made):
            assert sbuf.pos == 3 and sbuf.full
            # the functional forms over every row of the ring; a row shift on the rows side
            walk = P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, every, N, GAMMA, 2, 1.5, 1.5, row_shift=i)
            next_rows = walk[5]
            so, sn, do, dn = sbuf.observations, sbuf.next_observations, dbuf.frames, dbuf.next_frames
            out[f"walk{i}"] = list(walk)
            out[f"stacked{i}"] = [dict(x) for x in P.gather_load(so["image"], so["tactile"], every, sn["image"], sn["tactile"], row_shift=i,
                                                                 next_rows=next_rows)]
            out[f"frames{i}"] = [dict(x) for x in P.gather_load_frames(do["image"], do["tactile"], dbuf.ages, every, dn["image"], dn["tactile"],
                                                                       row_shift=i, next_rows=next_rows, frame_stack=fs)]
            g.check(f"after the functional forms of case {i}")
            # the buffers: every valid step of the frame-deduplicated ring, which includes the walks that wrap
            first, count = dbuf._valid_steps()
            t = np.repeat([(first + u) % T for u in range(count)], E)
            e = np.tile(np.arange(E), count)
            for name, buf in (("sbuf", sbuf), ("dbuf", dbuf)):
                batch = buf.sample(1, env=env, indices=(t, e))
                assert (batch.next_rows < batch.rows).any(), "no walk wraps the ring end"
                out[f"{name}{i}"] = [dict(batch.observations), batch.actions, dict(batch.next_observations), batch.dones, batch.rewards, batch.rows,
                                     batch.discounts, batch.next_rows]
            g.check(f"after the buffers of case {i}")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)


def test_memory_contract_of_td_target_rows(monkeypatch):
    heads = []
    for B, A_ in ((5, 1), (33, 3)):
        c = SC.make_inputs((16, (16,), (16,), A_), B, False, False, seed=4100 + 10 * B + A_)
        Fd, pi, qf, _ = c["arch"]
        head = m3l_amd.SACHead(Fd, A_, net_arch=dict(pi=list(pi), qf=list(qf)))
        head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}, strict=True)
        disc = torch.from_numpy((1.0 - np.random.default_rng(B).random(B)).astype(F32)).to(DEV)
        heads.append((head.to(DEV), {k: torch.from_numpy(c[k]).to(DEV) for k in ("x_next", "rewards", "dones", "noise_next")}, disc, c["ent_coef"]))

    def work(g):
        out = {}
        for i, (head, t, disc, ent) in enumerate(heads):
            out[f"rows{i}"] = head.td_target(t["x_next"], t["rewards"], t["dones"], disc.reshape(-1, 1), ent_coef=ent, noise=t["noise_next"])
            out[f"scalar{i}"] = head.td_target(t["x_next"], t["rewards"], t["dones"], 0.97, ent_coef=ent, noise=t["noise_next"])
        g.check("after td_target")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)
