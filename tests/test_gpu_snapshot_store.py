"""Device-resident snapshots (csrc/pg_snapshot.hip, procgen_store_* / procgen_fork_envs): env states
saved to, restored from and copied between envs in device memory.  A restored env must be
indistinguishable from its source -- frame, step data, level seeds, and every later step under the same
actions -- and the envs a call does not name must not notice it (they stay bit-exact against the CPU
oracle).  The host path (get_state / set_state) pins what a restored env reports."""
import hashlib

import numpy as np
import pytest

from oracle_lib import OracleEnv
from test_gpu_coinrun import KEYS, assert_same, gpu_obs
from test_gpu_games import make_gpu

pytestmark = pytest.mark.gpu

ALL = ["bigfish", "bossfight", "caveflyer", "chaser", "climber", "coinrun", "dodgeball", "fruitbot", "heist",
       "jumper", "leaper", "maze", "miner", "ninja", "plunder", "starpilot"]
OUT = ["rgb"] + KEYS
LATENT_KEYS = ("grid_size", "grid", "agent_pos", "exit_pos")


def assert_rows(g, a, h, b, what):
    """rows `a` of outputs g == rows `b` of outputs h, on every key"""
    for k in OUT:
        np.testing.assert_array_equal(g[k][a], h[k][b], err_msg="%s differs: %s" % (k, what))


def assert_latent(env, orc, what):
    """maze / miner: the latent info of env 3 equals env 0's, and envs 0-2 carry the oracle's"""
    info, lat = env.get_info_arrays(), orc.latent()
    for k in LATENT_KEYS:
        np.testing.assert_array_equal(info[k][3], info[k][0], err_msg="latent %s of env 3 vs env 0 %s" % (k, what))
        np.testing.assert_array_equal(info[k][:3], lat[k], err_msg="latent %s vs the oracle %s" % (k, what))


def raw_frames(env):
    """The frames the engine holds now, read past the sticky error check of observe()."""
    env._lib.libenv_observe(env._handle)
    return env._ob["rgb"].copy()


def warm(env, rng, steps, orc=None, upto=None):
    for t in range(1, steps + 1):
        act = rng.randint(0, 15, size=env.num).astype(np.int32)
        env.act(act)
        g = gpu_obs(env)
        if orc is not None:
            orc.step(act[:upto])
            assert_same(g, orc.observe(), t, idx=slice(0, upto))


# ---- 1: a forked env equals its source from then on; the other envs stay on the oracle's trajectory
@pytest.mark.parametrize("game", ALL)
def test_fork_equals_source_neighbours_untouched(game):
    num = 4
    env = make_gpu(num, game, num_levels=0, start_level=0, rand_seed=4)
    orc = OracleEnv(game, 3, num_levels=0, start_level=0, rand_seed=4)
    rng = np.random.RandomState(11)
    assert_same(gpu_obs(env), orc.observe(), 0, idx=slice(0, 3))
    warm(env, rng, 20, orc, 3)
    env.fork([0], [3])
    g = gpu_obs(env)
    assert_rows(g, 3, g, 0, "env 3 vs env 0 right after the fork")
    assert_same(g, orc.observe(), 20, idx=slice(0, 3))
    if game in ("maze", "miner"):
        assert_latent(env, orc, "right after the fork")
    for t in range(21, 101):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        act[3] = act[0]
        env.act(act)
        orc.step(act[:3])
        g = gpu_obs(env)
        assert_rows(g, 3, g, 0, "env 3 vs env 0 at step %d" % t)
        assert_same(g, orc.observe(), t, idx=slice(0, 3))
        if game in ("maze", "miner"):
            assert_latent(env, orc, "at step %d" % t)
    env.close()


# ---- 2: the same result as the host path
@pytest.mark.parametrize("game", ["coinrun", "maze", "miner", "bigfish"])
def test_fork_matches_host_set_state(game):
    num = 4
    kw = dict(num_levels=0, start_level=0, rand_seed=6)
    a, b = make_gpu(num, game, **kw), make_gpu(num, game, **kw)
    rng = np.random.RandomState(12)

    def both(t):
        ga, gb = gpu_obs(a), gpu_obs(b)
        assert_rows(ga, slice(None), gb, slice(None), "device fork vs host set_state at step %d" % t)
        if game in ("maze", "miner"):
            ia, ib = a.get_info_arrays(), b.get_info_arrays()
            for k in LATENT_KEYS:
                np.testing.assert_array_equal(ia[k], ib[k], err_msg="latent %s differs at step %d" % (k, t))

    for t in range(1, 21):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        a.act(act)
        b.act(act)
    both(20)
    a.fork([0, 1], [3, 2])
    st = b.get_state()
    st[3] = st[0]
    st[2] = st[1]
    b.set_state(st)
    both(20)
    for t in range(21, 81):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        a.act(act)
        b.act(act)
        both(t)
    a.close()
    b.close()


# ---- 3: destinations may overlap sources
def test_fork_overlapping_swap_and_fan_out():
    num = 4
    kw = dict(num_levels=0, start_level=0, rand_seed=7)
    env, ref = make_gpu(num, "coinrun", **kw), make_gpu(num, "coinrun", **kw)
    rng = np.random.RandomState(13)
    for _ in range(20):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        env.act(act)
        ref.act(act)
    before = gpu_obs(env)
    env.fork([1, 0, 0], [0, 1, 2])  # swaps 0 and 1, fans 0 out to 2
    perm = [1, 0, 0, 3]             # env k now holds what env perm[k] held
    assert_rows(gpu_obs(env), slice(None), before, perm, "frames and scalars after the overlapping fork")
    for t in range(21, 61):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        act[2] = act[1]             # both continue old env 0
        env.act(act)
        ra = act.copy()
        ra[0], ra[1] = act[1], act[0]   # the untouched engine steps old env k with the action its copy got
        ref.act(ra)
        assert_rows(gpu_obs(env), slice(None), gpu_obs(ref), perm, "step %d after the overlapping fork" % t)
    env.close()
    ref.close()


# ---- 4: rewind across episode ends, with the level prefetch and with parts
# num = 8 keeps a single-game batch in one chain whatever PROCGEN_MI355X_PARTS says (a part has at least 64
# envs), so the parts cases also run at 128 envs, where the batch does split
@pytest.mark.parametrize("game,num,nparts", [("jumper", 8, 1), ("jumper", 8, 2), ("bigfish", 8, 1), ("bigfish", 8, 2),
                                             ("jumper", 128, 2), ("bigfish", 128, 2)])
def test_rewind_across_episode_ends(game, num, nparts, monkeypatch):
    if game == "bigfish":
        monkeypatch.setenv("PROCGEN_MI355X_PREFETCH", "1")  # jumper prefetches by default
    if nparts > 1:
        monkeypatch.setenv("PROCGEN_MI355X_PARTS", str(nparts))
    env = make_gpu(num, game, num_levels=0, start_level=0, rand_seed=4)
    if num >= 64 * nparts:
        assert env.num_parts() == nparts
    rng = np.random.RandomState(14)
    for _ in range(20):
        env.act(rng.randint(0, 15, size=num).astype(np.int32))
    env.observe()
    store = env.snapshot_store(num)
    assert store.capacity == num and store.slot_bytes > 0
    store.save_all()
    acts = rng.randint(0, 15, size=(150, num)).astype(np.int32)

    def keep(g):  # whole frames for a small batch, a digest of them for a large one
        if num > 8:
            g["rgb"] = hashlib.sha1(g["rgb"].tobytes()).hexdigest()
        return g

    rec = [keep(gpu_obs(env))]
    for act in acts:
        env.act(act)
        rec.append(keep(gpu_obs(env)))
    assert sum(int(r["first"].sum()) for r in rec[1:]) > 0, "no episode ended in the recorded run"
    store.load_all()
    for t in range(151):
        if t:
            env.act(acts[t - 1])
        g = keep(gpu_obs(env))
        for k in OUT:
            np.testing.assert_array_equal(g[k], rec[t][k], err_msg="%s differs %d steps after the rewind" % (k, t))
    store.close()
    env.close()


# ---- 5: mixed batch: a state only enters a slot of its own game
def test_mixed_batch_same_game_only():
    from procgen_amd import ProcgenError
    names = "maze,heist,bossfight,starpilot"
    num = 8
    env = make_gpu(num, names, num_levels=0, start_level=0, rand_seed=8)
    rng = np.random.RandomState(15)
    warm(env, rng, 10)
    store = env.snapshot_store(2)
    store.save([0], [0])
    store.load([0], [4])  # env 4 plays maze too
    g = gpu_obs(env)
    assert_rows(g, 4, g, 0, "env 4 vs env 0 right after the load")
    for t in range(11, 41):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        act[4] = act[0]
        env.act(act)
        g = gpu_obs(env)
        assert_rows(g, 4, g, 0, "env 4 vs env 0 at step %d" % t)
    frames = raw_frames(env)
    with pytest.raises(ProcgenError):
        store.load([0], [1])  # env 1 plays heist
    np.testing.assert_array_equal(raw_frames(env), frames)
    env.close()


# ---- 6: what the host rejects, before any env is touched
def _unfilled(env, st):
    st.load([1], [0])


def _slot_high(env, st):
    st.save([0], [4])


def _slot_negative(env, st):
    st.save([0], [0])
    st.load([-1], [0])


def _env_high(env, st):
    st.save([4], [0])


def _env_negative_fork(env, st):
    env.fork([0], [-1])


def _fork_src_high(env, st):
    env.fork([4], [0])


def _dup_load_envs(env, st):
    st.save([0, 1], [0, 1])
    st.load([0, 1], [2, 2])


def _dup_fork_dst(env, st):
    env.fork([0, 1], [2, 2])


def _dup_save_slots(env, st):
    st.save([0, 1], [2, 2])


def _after_close(env, st):
    st.save([0], [0])
    st.close()
    st.load([0], [1])


@pytest.mark.parametrize("bad", [_unfilled, _slot_high, _slot_negative, _env_high, _env_negative_fork, _fork_src_high,
                                 _dup_load_envs, _dup_fork_dst, _dup_save_slots, _after_close])
def test_rejections(bad):
    from procgen_amd import ProcgenError
    num = 4
    env = make_gpu(num, "coinrun", num_levels=0, start_level=0, rand_seed=9)
    rng = np.random.RandomState(16)
    warm(env, rng, 3)
    st = env.snapshot_store(4)
    frames = raw_frames(env)
    with pytest.raises(ProcgenError):
        bad(env, st)
    np.testing.assert_array_equal(raw_frames(env), frames)
    env.close()
    with pytest.raises(ProcgenError):  # the store died with its env
        st.save([0], [0])
    # duplicate sources are fine, on a fresh handle
    env = make_gpu(num, "coinrun", num_levels=0, start_level=0, rand_seed=9)
    st = env.snapshot_store(4)
    st.save([0, 0], [0, 1])
    st.load([0, 0, 1], [1, 2, 3])
    env.fork([0, 0], [1, 2])
    g = gpu_obs(env)
    for e in (1, 2, 3):
        assert_rows(g, e, g, 0, "env %d vs env 0" % e)
    env.close()


# ---- 7: a device-resident env
def test_fork_device_buffers():
    import torch
    num = 8
    env = make_gpu(num, "coinrun", num_levels=0, start_level=0, rand_seed=10, device_buffers=True)
    rng = np.random.RandomState(17)
    src, dst = [0, 1], [5, 6]

    def step(mirror):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        if mirror:
            act[dst] = act[src]
        d_act = torch.from_numpy(act).to("cuda")
        torch.cuda.synchronize()  # the engine's stream is not torch's
        env.act_device(d_act.data_ptr())
        env.wait()

    def check(what):
        o = env.read_envs(src + dst)
        for k in OUT:
            np.testing.assert_array_equal(o[k][2:], o[k][:2], err_msg="%s differs %s" % (k, what))

    for _ in range(20):
        step(False)
    env.fork(src, dst)
    check("right after the fork")
    for t in range(30):
        step(True)
        check("%d steps after the fork" % (t + 1))
    env.close()


# ---- 8: use_generated_assets: the env's own background travels with its state
def test_fork_generated_assets():
    num = 4
    env = make_gpu(num, "coinrun", num_levels=0, start_level=0, rand_seed=11, use_generated_assets=True)
    rng = np.random.RandomState(18)
    warm(env, rng, 5)
    env.fork([0], [3])
    g = gpu_obs(env)
    assert_rows(g, 3, g, 0, "env 3 vs env 0 right after the fork")
    for t in range(6, 26):
        act = rng.randint(0, 15, size=num).astype(np.int32)
        act[3] = act[0]
        env.act(act)
        g = gpu_obs(env)
        assert_rows(g, 3, g, 0, "env 3 vs env 0 at step %d" % t)
    env.close()
