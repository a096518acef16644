"""The memory contract (tests/memguard.py, test_memory_contract_gpu.py) for the entry points of the random-shift augmentation:
m3l_replay_gather_load_shift and m3l_replay_gather_load_frames_shift write nothing outside the outputs they were handed, and no output byte
depends on what those outputs held before.  Every output of theirs is allocated inside m3l_amd, so inside a MemGuard it lies between two guards
and is pre-filled with 0xFF (NaN) or 0x00: equal bits across the fills and intact guards.

Shapes: those of test_replay_shift_gpu.py (shift_cases.CONFIGS) — the 16-byte and the element-per-lane forms of both modalities, uint8 and
float32 stores — on a ring of 7 steps of 2 environments that has wrapped, with the injected shifts of that test: every shift of the range in
each half, the corners, and out-of-range entries up to INT32_MIN / INT32_MAX.  One list of rows and two, with a row shift; stacked and
frame-deduplicated, two stores and one."""
import numpy as np
import pytest
import torch

import memguard as MG
import shift_cases as SH

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402

DEV = "cuda:0"
T, E, A = SH.T, SH.E, SH.A


def _filled(cfg, seed, **kw):
    fs, image_hw, tactile_hw, S, dtypes, pads = cfg
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=seed)
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    buf = m3l_amd.DeviceReplayBuffer(T * E, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, device=DEV,
                                     random_shift=dict(image=pads[0], tactile=pads[1]), **kw)
    for k in range(SH.N_ADDS):
        buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
                st["dones"][k], st["infos"][k])
    return buf


def test_memory_contract_of_the_shift_entry_points(monkeypatch):
    single = dict(optimize_memory_usage=True, handle_timeout_termination=False)
    made = []
    for i, name in enumerate(sorted(SH.CONFIGS)):
        cfg = SH.CONFIGS[name]
        shifts = torch.from_numpy(SH.injected_shifts(cfg[5])).to(DEV)          # the whole list, its out-of-range entries included
        made.append((cfg, shifts, _filled(cfg, 600 + i), _filled(cfg, 600 + i, frame_dedup=True), _filled(cfg, 600 + i, **single),
                     _filled(cfg, 600 + i, frame_dedup=True, **single)))

    def work(g):
        out = {}
        for i, (cfg, shifts, sbuf, dbuf, sbuf1, dbuf1) in enumerate(made):
            fs, pads, B = cfg[0], cfg[5], shifts.shape[0]
            assert sbuf.pos == 3 and sbuf.full and B > 3 * T * E
            every = torch.arange(B, dtype=torch.int64, device=DEV) % (T * E)          # every row of the ring, more than once
            other = torch.flip(every, (0,)).contiguous()
            so, sn, do, dn = sbuf.observations, sbuf.next_observations, dbuf.frames, dbuf.next_frames
            # the functional forms over every row of the ring: one list with a row shift, and two lists
            for tag, kw in (("one", dict(row_shift=i + 1)), ("two", dict(row_shift=i + 1, next_rows=other))):
                out[f"stacked_{tag}{i}"] = [dict(x) for x in P.gather_load(so["image"], so["tactile"], every, sn["image"], sn["tactile"], shifts=shifts,
                                                                           shift_pad=pads, **kw)]
                out[f"frames_{tag}{i}"] = [dict(x) for x in P.gather_load_frames(do["image"], do["tactile"], dbuf.ages, every, dn["image"],
                                                                                 dn["tactile"], shifts=shifts, shift_pad=pads, frame_stack=fs, **kw)]
            g.check(f"after the functional forms of case {i}")
            # the buffers over every valid step of theirs, with injected and with drawn shifts
            for bname, buf in (("sbuf", sbuf), ("dbuf", dbuf), ("sbuf1", sbuf1), ("dbuf1", dbuf1)):
                first, count = buf._valid_steps()
                t = np.resize(np.repeat([(first + u) % T for u in range(count)], E), B)
                e = np.resize(np.tile(np.arange(E), count), B)
                batch = buf.sample(1, indices=(t, e), shifts=shifts)
                out[f"{bname}{i}"] = [dict(batch.observations), batch.actions, dict(batch.next_observations), batch.dones, batch.rewards, batch.rows]
                torch.manual_seed(i)
                drawn = buf.sample(1, indices=(t, e))
                out[f"{bname}_drawn{i}"] = [dict(drawn.observations), dict(drawn.next_observations), buf.last_shifts]
            g.check(f"after the buffers of case {i}")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)
