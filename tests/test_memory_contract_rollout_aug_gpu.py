"""The memory contract (tests/memguard.py, test_memory_contract_gpu.py) for the rollout's new gather entry points:
m3l_rollout_gather_load_shift, m3l_rollout_gather_load_frames and m3l_rollout_gather_load_frames_shift write nothing outside the outputs they
were handed, and no output byte depends on what those outputs held before.  Every output of theirs is allocated inside m3l_amd, so inside a
MemGuard it lies between two guards and is pre-filled with 0xFF (NaN) or 0x00: equal bits across the fills and intact guards.

Shapes: those of test_rollout_aug_gpu.py (shift_cases.CONFIGS) — the 16-byte and the element-per-lane forms of both modalities, uint8 and
float32 stores — on the second of two consecutive rollouts of 7 steps of 2 environments, with the injected shifts of that test: every shift of the
range, the corners, and out-of-range entries up to INT32_MIN / INT32_MAX.  The functional forms and the buffer, injected and drawn shifts."""
import pytest
import torch

import memguard as MG
import rollout_aug_cases as RA

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import rollout as R  # noqa: E402

DEV = "cuda:0"
E, A, T = RA.E, RA.A, 7


def _filled(name, seed, **kw):
    fs, image_hw, tactile_hw, S, dtypes, pads = RA.CONFIGS[name]
    ro = RA.make_rollouts(name, T, seed=seed)
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    buf = m3l_amd.DeviceRolloutBuffer(T, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, device=DEV, **kw)
    for r in (0, 1):
        buf.reset()
        for k in range(r * T, (r + 1) * T):
            buf.add({key: v[k] for key, v in ro["obs"].items()}, ro["actions"][k], ro["rewards"][k], ro["episode_start"][k], ro["values"][k],
                    ro["log_probs"][k])
        buf.compute_returns_and_advantage(ro["last_values"][r], ro["dones"][r])
    return buf


def test_memory_contract_of_the_rollout_augmentation_entry_points(monkeypatch):
    made = []
    for i, name in enumerate(sorted(RA.CONFIGS)):
        pads = RA.CONFIGS[name][5]
        shift = dict(image=pads[0], tactile=pads[1])
        shifts = torch.from_numpy(RA.injected_shifts(pads)).to(DEV)          # the whole list, its out-of-range entries included
        made.append((name, shifts, _filled(name, 700 + i, random_shift=shift), _filled(name, 700 + i, frame_dedup=True, random_shift=shift),
                     _filled(name, 700 + i, frame_dedup=True)))

    def work(g):
        out = {}
        for i, (name, shifts, sbuf, dbuf, dplain) in enumerate(made):
            fs, pads, B = RA.CONFIGS[name][0], RA.CONFIGS[name][5], shifts.shape[0]
            assert sbuf.full and dbuf.full and B > 3 * T * E
            every = torch.arange(B, dtype=torch.int64, device=DEV) % (T * E)          # every flat index, more than once
            so, fr = sbuf.observations, dbuf.frames
            # the functional forms: the three new entry points
            out[f"shift{i}"] = dict(R.gather_load(so["image"], so["tactile"], every, shifts=shifts, shift_pad=pads))
            out[f"frames{i}"] = dict(R.gather_load_frames(fr["image"], fr["tactile"], dbuf.ages, every, fs))
            out[f"frames_shift{i}"] = dict(R.gather_load_frames(fr["image"], fr["tactile"], dbuf.ages, every, fs, shifts=shifts, shift_pad=pads))
            g.check(f"after the functional forms of case {i}")
            # the buffers over every flat index, with injected and with drawn shifts, in one batch and in minibatches
            idx = every.cpu().numpy()
            for bname, buf in (("sbuf", sbuf), ("dbuf", dbuf)):
                batch, = list(buf.get(indices=idx, shifts=shifts))
                out[f"{bname}{i}"] = [dict(batch.x)] + list(batch[1:])
                torch.manual_seed(i)
                drawn = list(buf.get(batch_size=B // 2 + 1, indices=idx))
                out[f"{bname}_drawn{i}"] = [[dict(b.x)] + list(b[1:]) for b in drawn] + [buf.last_shifts]
            batch, = list(dplain.get(indices=idx))
            out[f"dplain{i}"] = [dict(batch.x)] + list(batch[1:])
            g.check(f"after the buffers of case {i}")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)
