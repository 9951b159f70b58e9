"""GPU suite of the life of a ``DeviceLoop`` (social_gym/device_loop.py) under ``BatchedSocialNavGym``: a second device reset releases the
first loop before the next is built, a construction that fails behind ``stream_create``, ``close()`` twice, a Gym dropped without
``close()``, and ``lookahead_device`` from a caller's own stream.  8 hybrid worlds x 5 humans, two staged episodes a world refilled every 4 steps, episodes of at most 12 steps: the refill stream
is busy when the loop goes."""
import gc

import pytest

pytestmark = pytest.mark.gpu

W, N = 8, 5


def _env():
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    cfg = _config("hybrid_scenario", human_num=N)
    cfg.set("env", "time_limit", "3")
    env = BatchedSocialNavGym(cfg, W)
    env.STAGE_DEPTH, env.REFILL_EVERY = 2, 4
    env.reset(phase="train", first_case=0, device=True)
    return env


def _step(env, steps, seed=7):
    import torch

    gen = torch.Generator(device="cuda").manual_seed(seed)
    ended = 0
    for _ in range(steps):
        _, _, term, trunc, _ = env.step_device(torch.randn(W, 2, device="cuda", generator=gen) * 0.5)
        ended += int((term | trunc).sum().item())
    return ended


def test_a_second_device_reset_releases_the_first_loop_and_starts_a_new_one():
    env = _env()
    assert _step(env, 40) >= W                         # every world ran out of time at least once: staged episodes were consumed and refilled
    first = env._dl
    assert first.depth == 2 and not first.released and int(first.epoch.min()) > 0
    env.reset(phase="train", first_case=0, device=True)
    second = env._device_loop_state()
    assert first.released and second is not first and env._dl is second and not second.released and second.cw is env.cw
    assert int(second.counter.abs().sum()) == 0 and int(second.epoch.abs().sum()) == 0
    _step(env, 3)
    assert int(second.counter.max()) == 3              # the new loop steps (a world whose episode ended on the way counts from 0 again)
    env.close()
    assert second.released and env._dl is None


def test_a_construction_that_fails_destroys_the_library_stream(monkeypatch):
    from social_navigation_pyenvs_amd import _lib

    created, destroyed = [], []
    create, destroy = _lib.stream_create, _lib.stream_destroy

    def failing_event():
        raise RuntimeError("no event today")

    env = _env()
    monkeypatch.setattr(_lib, "stream_create", lambda **kw: created.append(create(**kw)) or created[-1])
    monkeypatch.setattr(_lib, "stream_destroy", lambda s: destroyed.append(s) or destroy(s))
    monkeypatch.setattr(_lib, "Event", failing_event)
    with pytest.raises(RuntimeError, match="no event today"):
        env._device_loop_state()
    assert len(created) == 1 and destroyed == created and env._dl is None
    monkeypatch.undo()
    _step(env, 3)                                      # the same Gym builds its loop once the cause is gone
    assert not env._dl.released and int(env._dl.counter.max()) == 3
    env.close()


def test_close_twice_is_harmless():
    env = _env()
    _step(env, 5)
    loop = env._dl
    env.close()
    env.close()
    assert loop.released and env._dl is None
    loop.release()


def test_a_dropped_gym_leaves_the_process_able_to_build_the_next():
    import torch

    for _ in range(3):
        env = _env()
        assert _step(env, 16) >= W
        loop = env._dl
        del env
        gc.collect()
        assert loop.released                           # the Gym's __del__ drained and destroyed the refill stream
        del loop
    torch.cuda.synchronize()


def test_lookahead_device_from_a_callers_stream_equals_the_default_stream():
    import numpy as np
    import torch

    env = _env()
    _step(env, 5)
    acts = np.stack([np.cos(np.arange(9) * 0.7), np.sin(np.arange(9) * 0.7)], -1).astype(np.float32)
    rot0, rew0 = (t.clone() for t in env.lookahead_device(acts))
    torch.cuda.synchronize()
    mine = torch.cuda.Stream()
    with torch.cuda.stream(mine):
        rot1, rew1 = env.lookahead_device(acts)
        rot1, rew1 = rot1.clone(), rew1.clone()        # read on the caller's stream: ordered behind the library's by the scope
    with torch.cuda.stream(env.device_stream()):
        rot2, rew2 = env.lookahead_device(acts)
    torch.cuda.synchronize()
    assert rot0.shape == (W, 9, N, 13) and rew0.shape == (W, 9) and bool(torch.isfinite(rot0).all())
    for rot, rew in ((rot1, rew1), (rot2, rew2)):
        assert torch.equal(rot, rot0) and torch.equal(rew, rew0)
    env.close()
