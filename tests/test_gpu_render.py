"""Frames on the device (cz_render_device, k_render): exact against `render.host_frame` of the oracle's records with a random-byte
sprite sheet, on every kernel instance, on the dword and the byte store path, in every subset of the two outputs, at every tile
size, with the master smaller and larger than the tile, over ranges, behind a step on the stream, inside a caller's graph,
sharded, and through the host convenience."""
import numpy as np
import pytest

from cooking_zoo_amd import _native, render, soa
from grid_common import CASES, checkpoints
from render_common import FORM_SUBSETS, FORMS, RenderBufs, random_sheet
from vec_common import COOP, CallerStream, env_of, instance, oracle_for, policy, strip, tables_of

pytestmark = pytest.mark.gpu

RUNS = [(name, False) for name in CASES] + [("coop_test", True)]
VIS = 0b0110


@pytest.mark.parametrize("name,spawn", RUNS, ids=[f"{n}{'-spawn' if s else ''}" for n, s in RUNS])
def test_every_instance_state_and_form(name, spawn):
    """set_state(oracle records) then the render call at P = 8 (row pitch a multiple of 4): every checkpoint in both forms, the
    last one in all three subsets of the outputs"""
    n = 6
    tables, points = checkpoints(name, n, spawn)
    env = env_of(tables)
    assert instance(env) == CASES[name][5], "the case runs on another kernel instance"
    env.reset(return_obs=False)
    sheet = random_sheet(8)
    env.load_sprites(sheet)
    assert (env.dims.W * 8 * 3) % 4 == 0
    b = RenderBufs(env, n, 8)
    if spawn:
        assert ((points[:, :, soa.W_STATUS] >> 8) & 0xF).any(), "no checkpoint has a despawned agent"
    for k, recs in enumerate(points):
        env.set_state(recs)
        want = render.host_frame(env.dims, recs, 8, sheet, VIS)
        for forms in (FORM_SUBSETS if k == len(points) - 1 else [FORMS]):
            b.fill()
            env.render_device(P=8, vis=VIS, **b.args(forms))
            b.check(f"{name} checkpoint {k} forms={forms}", forms, want)
    assert env.frame_shape(8) == (env.dims.H * 8, env.dims.W * 8, 3)
    env.close()


@pytest.mark.parametrize("spawn", [False, True])
def test_byte_path_on_a_seven_wide_level(spawn):
    """P = 5 on coop_test (7 x 7): the row pitch 105 is no multiple of 4"""
    n = 7
    tables, points = checkpoints("coop_test", n, spawn)
    env = env_of(tables)
    assert env.dims.W == 7 and (env.dims.W * 5 * 3) % 4 != 0
    env.reset(return_obs=False)
    sheet = random_sheet(12)
    env.load_sprites(sheet)
    b = RenderBufs(env, n, 5)
    for k, recs in enumerate(points):
        env.set_state(recs)
        want = render.host_frame(env.dims, recs, 5, sheet, 1)
        for forms in FORM_SUBSETS:
            b.fill()
            env.render_device(P=5, vis=1, **b.args(forms))
            b.check(f"checkpoint {k} forms={forms}", forms, want)
    env.close()


def test_every_tile_size():
    """one env of the smallest level at every P from 4 to 96: the C geometry against render.geometry, and every draw size"""
    tables, points = checkpoints("crowded_6x5", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    sheet = random_sheet(16)
    env.load_sprites(sheet)
    env.set_state(points[-1])
    rec = points[-1][2:3]
    for P in range(4, 97):
        b = RenderBufs(env, 1, P)
        env.render_device(P=P, vis=VIS, env_begin=2, env_count=1, **b.args(FORMS))
        b.check(f"P = {P}", FORMS, render.host_frame(env.dims, rec, P, sheet, VIS))
        for f in FORMS:
            b.buf[f].free()
    env.close()


@pytest.mark.parametrize("M,P", [(16, 80), (32, 8), (1, 9), (128, 128)])
def test_master_resolution_differs_from_the_tile(M, P):
    tables, points = checkpoints("coop_test", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[-1])
    sheet = random_sheet(M)
    env.load_sprites(sheet)
    b = RenderBufs(env, 2, P)
    env.render_device(P=P, env_begin=1, env_count=2, **b.args(FORMS))
    b.check(f"M = {M}, P = {P}", FORMS, render.host_frame(env.dims, points[-1][1:3], P, sheet, 0))
    env.close()


def test_a_second_sheet_replaces_the_first():
    tables, points = checkpoints("coop_test", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[0])
    b = RenderBufs(env, 6, 8)
    for sheet in (random_sheet(8, 1), random_sheet(20, 2), render.builtin_sprites(16)):
        env.load_sprites(sheet)
        b.fill()
        env.render_device(P=8, **b.args(FORMS))
        b.check(f"sheet M = {sheet.shape[1]}", FORMS, render.host_frame(env.dims, points[0], 8, sheet, 0))
    env.close()


def test_ranges_and_refusals():
    n = 13
    tables, points = checkpoints("coop_test", n)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[-1])
    L = _native.lib()
    assert L.cz_render_sprites() == render.N_SPRITES
    b = RenderBufs(env, 5, 8)
    p = lambda f: b.buf[f].ptr
    assert L.cz_render_device(env._h, 0, 5, 8, 0, p("rgb8"), None) != 0 and "no sprite sheet" in L.cz_last_error(env._h).decode()
    sheet = random_sheet(8)
    for args, msg in (((None, render.N_SPRITES, 8), "null"), ((sheet.ctypes.data, render.N_SPRITES - 1, 8), "sprites"),
                      ((sheet.ctypes.data, render.N_SPRITES, 0), "M ="), ((sheet.ctypes.data, render.N_SPRITES, 129), "M =")):
        assert L.cz_load_sprites(env._h, *args) != 0, f"{args} was accepted"
        assert msg in L.cz_last_error(env._h).decode()
    env.load_sprites(sheet)
    env.render_device(P=8, env_begin=3, env_count=5, **b.args(FORMS))
    b.check("envs 3..7", FORMS, render.host_frame(env.dims, points[-1][3:8], 8, sheet, 0))
    b.fill()
    env.render_device(P=8, env_begin=7, env_count=0, **b.args(FORMS))
    b.check("env_count = 0", (), None)
    for args, msg in (((0, 5, 3, 0, p("rgb8"), None), "P ="), ((0, 5, 129, 0, p("rgb8"), None), "P ="), ((0, 5, 8, 0, None, None), "null"),
                      ((0, 5, 8, 0, p("rgb8") + 2, None), "aligned"), ((0, 5, 8, 0, None, p("chw32") + 4), "aligned"),
                      ((10, 5, 8, 0, p("rgb8"), None), "range"), ((-1, 2, 8, 0, p("rgb8"), None), "range"),
                      ((0, n + 1, 8, 0, p("rgb8"), None), "range")):
        assert L.cz_render_device(env._h, *args) != 0, f"{args} was accepted"
        text = L.cz_last_error(env._h).decode()
        assert msg in text, f"{args}: message {text!r}"
    with pytest.raises(_native.NativeError, match="null"):
        env.render_device()
    b.check("after the refusals", (), None)
    assert np.array_equal(env.get_state(), points[-1]), "the render call wrote a record"
    env.close()


def closed_loop_env(n=9):
    tables = tables_of(n, **dict(COOP, max_steps=7))
    env = env_of(tables)
    A = env.num_agents
    d = dict(act=env.alloc((n, A), np.int32), rew=env.alloc((n, A), np.float64), term=env.alloc((n, A), np.uint8),
             trunc=env.alloc((n, A), np.uint8))
    return env, d


def test_stream_order_behind_a_step():
    """step_device then render_device with no synchronisation in between, 12 steps with auto-resets onto other layouts"""
    n = 9
    env, d = closed_loop_env(n)
    orc, pol = oracle_for(env), policy(env, 3)
    env.reset(return_obs=False)
    orc.reset()
    sheet = random_sheet(8)
    env.load_sprites(sheet)
    b = RenderBufs(env, n, 8)
    for t in range(12):
        acts = pol.act(orc.records)
        d["act"].from_host(acts)
        b.fill()
        env.step_device(d["act"], None, d["rew"], d["term"], d["trunc"])
        env.render_device(P=8, vis=2, **b.args(FORMS))
        orc.step(acts, want_obs=False)
        pol.observe_result(orc.records)
        b.check(f"step {t}", FORMS, render.host_frame(env.dims, orc.records, 8, sheet, 2))
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"step {t}: records"
    assert int(orc.records[:, soa.W_EPISODE].min()) >= 1, "no auto-reset"
    env.close()


def test_captured_into_a_callers_graph():
    """the pair captured once and replayed 4 times shows the state of each replay"""
    n = 9
    env, d = closed_loop_env(n)
    orc, pol = oracle_for(env), policy(env, 4)
    env.reset(return_obs=False)
    orc.reset()
    sheet = random_sheet(8)
    env.load_sprites(sheet)
    b = RenderBufs(env, n, 8)
    before = env.get_state()
    cs = CallerStream(env)
    with cs.capture():
        env.step_device(d["act"], None, d["rew"], d["term"], d["trunc"])
        env.render_device(P=8, **b.args(FORMS))
    assert np.array_equal(env.get_state(), before), "capturing executed something"
    b.check("after the capture", (), None)
    for r in range(4):
        acts = pol.act(orc.records)
        d["act"].from_host(acts)
        cs.replay()
        cs.sync()
        orc.step(acts, want_obs=False)
        pol.observe_result(orc.records)
        b.check(f"replay {r}", FORMS, render.host_frame(env.dims, orc.records, 8, sheet, 0))
        assert np.array_equal(strip(env.get_state()), strip(orc.records)), f"replay {r}: records"
    cs.close()
    env.close()


def test_sharded_equals_the_host_model():
    from cooking_zoo_amd.sharded import ShardedVecEnv
    n = 11
    level, meta, agents, recipes, scheme, _inst, _steps = CASES["crowded_6x5"]
    tables, points = checkpoints("crowded_6x5", n)
    sh = ShardedVecEnv(n, level, meta, agents, 241, recipes, device_ids=[0, 0, 0], action_scheme=scheme, num_layouts=4)
    assert len({s.num_envs for s in sh.shards}) > 1, "the shards are equal"
    sh.reset(return_obs=False)
    sh.set_state(points[-1])
    sheet = random_sheet(8)
    sh.load_sprites(sheet)
    h, w, _ = sh.frame_shape(8)
    want = render.host_frame(tables.dims, points[-1], 8, sheet, VIS)
    d_rgb, d_chw = sh.alloc((h, w, 3), np.uint8), sh.alloc((3, h, w), np.float32)
    sh.render_device(d_rgb, d_chw, P=8, vis=VIS)
    sh.sync()
    assert np.array_equal(d_rgb.to_host(), want), "rgb8: the shards differ from the host model"
    assert np.array_equal(d_chw.to_host().view(np.uint32), render.to_chw32(want).view(np.uint32)), "chw32"
    assert np.array_equal(sh.render(2, 8, P=8, vis=VIS), want[2:10]), "the host form over a range that spans shards"
    sh.close()


def test_host_convenience():
    tables, points = checkpoints("limit_8x31", 6)
    env = env_of(tables)
    env.reset(return_obs=False)
    env.set_state(points[1])
    f = env.render(env_begin=2, env_count=3, P=6, vis=1)                  # loads the builtin sheet on first use
    assert f.dtype == np.uint8 and f.shape == (3,) + env.frame_shape(6)
    assert np.array_equal(f, render.host_frame(env.dims, points[1][2:5], 6, render.builtin_sprites(16), 1))
    assert env.render(env_count=0).shape == (0,) + env.frame_shape(16)
    env.close()


def test_facade_render_on_the_device():
    """CookingEnvironment.render(): the (H * 80, W * 80, 3) frame of its one env with the constructor's agent_visualization, after
    the reset and after a few steps; the AEC facade forwards"""
    import random
    from cooking_zoo_amd.environment.cooking_env import env as aec_env, parallel_env
    random.seed(5)
    kw = dict(level="coop_test", meta_file="example", num_agents=2, max_steps=20, recipes=["TomatoLettuceSalad", "CarrotBanana"],
              agent_visualization=["robot", "human"], action_scheme="scheme3")
    e = parallel_env(**kw)
    e.reset()
    sheet = render.builtin_sprites(16)
    for t in range(4):
        frame = e.render()
        dims = e._vec.dims
        assert frame.dtype == np.uint8 and frame.shape == (dims.H * 80, dims.W * 80, 3)
        assert np.array_equal(frame, render.host_frame(dims, e._vec.get_state()[0], 80, sheet, 0b01)), f"step {t}"
        e.step({a: 1 + (t + i) % 4 for i, a in enumerate(e.agents)})
    e.close()
    a = aec_env(**kw)
    a.reset()
    assert np.array_equal(a.render(), render.host_frame(a._core._vec.dims, a._core._vec.get_state()[0], 80, sheet, 0b01))
    a.close()
