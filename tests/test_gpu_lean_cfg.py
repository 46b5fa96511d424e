"""GPU: the lean one-step kernels with the handle's recipe count, end condition and walk_touches fixed at compile time
(k_step_lean_cfg, the rows of CZ_LEAN_CFGS in cz_kernels.h) against the oracle and against the generic kernel (CZ_LEAN=0).

Every row a handle can select is stepped at the shapes at which a one-wave-per-env kernel can go wrong - 9 envs (a full workgroup of
eight plus a partial one whose spare waves shadow the last env) and 1 env - with max_steps = 3 over 12 steps and a pool of two
layouts, so that truncation, the reset pass and the move to a layout with another descriptor row all fall inside the run.
Observations, rewards, flags, records and statistics are compared bit for bit; cz_diag_last_step_variant says which kernel ran:
-1 not a lean kernel, 0 k_step_lean, 0x100 | R | end_all << 4 | walk_touches << 5 a k_step_lean_cfg.  The golden episodes of
BASELINE configs 1 and 2 - dishes are delivered and terminate episodes there, so the reward of a changed recipe mark runs with R
fixed - are replayed through the same kernels.  The last test counts the rows that ran."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from cooking_zoo_amd import _native, soa
from golden_io import GoldenSet
from gpu_common import handle_for_set, strip_golden
from vec_common import bits, lean, make_env, oracle_for, strip

pytestmark = pytest.mark.gpu

make = functools.partial(make_env, num_layouts=16)          # coop_test, two agents, 30 steps; 16 layouts

HEADER = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc", "cz_kernels.h")


def instantiated_rows():
    """the rows of CZ_LEAN_CFGS: (agents, scheme, recipes, end_all, walk_touches)"""
    src = open(HEADER).read()
    m = re.search(r"#define CZ_LEAN_CFGS\(X\)((?:.*\\\n)*.*)\n", src)
    return [tuple(int(v) for v in row) for row in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", m.group(1))]


ROWS = instantiated_rows()
RAN = set()
BOOK = ["TomatoLettuceSalad", "CarrotBanana", "TomatoSalad", "MashedCarrotBanana"]
# (level, meta file) by agent count: the 7x7 level of the headline workload; three agents need a level with three spawn areas
LEVEL = {1: ("coop_test", "example"), 2: ("coop_test", "example"), 3: ("edge_8x8", "edge"), 4: ("crowded_6x5", "crowded_6x5")}


def variant(h):
    L = _native.lib()
    L.cz_diag_last_step_variant.restype = C.c_int32
    L.cz_diag_last_step_variant.argtypes = [C.c_void_p]
    return int(L.cz_diag_last_step_variant(h))


def code(R, end_all, walk_touches):
    return 0x100 | R | (end_all << 4) | (walk_touches << 5)


def run_against_oracle(n, agents, scheme, R, end_all, expect, T=12, max_steps=3):
    """T steps of one handle with a lean kernel, one with CZ_LEAN=0 and the oracle; -> the variants the lean handle reported"""
    level, meta = LEVEL[agents]
    kw = dict(level=level, meta=meta, agents=agents, recipes=BOOK[:R], scheme="scheme%d" % scheme, max_steps=max_steps,
              num_layouts=2, end_condition_all_dishes=bool(end_all))
    with lean(True):
        ea = make(n, **kw)
    with lean(False):
        eb = make(n, **kw)
    assert len(ea.layouts) == 2 and ea.num_recipes == R
    orc = oracle_for(ea)
    ea.reset(return_obs=False), eb.reset(return_obs=False), orc.reset()
    rng = np.random.default_rng(1000 * n + 100 * agents + 10 * R + end_all)
    A, F = ea.num_agents, ea.F
    bufs = [(e.alloc((n, A), np.int32), e.alloc((n, A, F), np.float64), e.alloc((n, A), np.float64), e.alloc((n, A), np.uint8),
             e.alloc((n, A), np.uint8)) for e in (ea, eb)]
    seen, layouts_seen = set(), set()
    st = dict(env_steps=0, episodes=0, length_sum=0, truncations=0, terminations=0, recipes_completed=[0] * 4)
    cur, ret_sum = np.zeros((n, A)), np.zeros(4)
    for t in range(T):
        acts = rng.integers(0, ea.n_actions, size=(n, A), dtype=np.int32)
        outs = []
        for e, (d_act, *o) in zip((ea, eb), bufs):
            d_act.from_host(acts)
            e.step_device(d_act, *o)
            outs.append([b.to_host() for b in o] + [e.get_state()])
        seen.add(variant(ea._h))
        assert variant(eb._h) == -1
        for k, (u, v) in enumerate(zip(*outs)):
            assert u.tobytes() == v.tobytes(), f"step {t}: output {k} differs between the lean and the generic kernel"
        was_done = (orc.records[:, soa.W_STATUS] & 1).astype(bool)
        oo, ro, to, uo = orc.step(acts)
        obs, rew, term, trunc, rec = outs[0]
        assert np.array_equal(bits(obs), bits(oo)), f"step {t}: obs vs oracle"
        assert np.array_equal(bits(rew), bits(ro)), f"step {t}: reward vs oracle"
        assert np.array_equal(term, to) and np.array_equal(trunc, uo), f"step {t}: flags vs oracle"
        assert np.array_equal(strip(rec), orc.records), f"step {t}: state vs oracle"
        layouts_seen |= set(int(v) for v in orc.records[:, soa.W_LAYOUT])
        for e in range(n):                                   # the statistics the device keeps, from the oracle's run
            if was_done[e]:
                continue
            st["env_steps"] += 1
            cur[e] += ro[e]
            if orc.records[e, soa.W_STATUS] & 1:
                st["episodes"] += 1
                st["length_sum"] += int(orc.records[e, soa.W_T])
                st["truncations"] += int(uo[e, 0])
                st["terminations"] += int(to[e, 0])
                for a in range(A):
                    ret_sum[a] += cur[e, a]
                    st["recipes_completed"][a] += (int(orc.records[e, soa.W_MARKS]) >> (8 * a)) & 1
                cur[e] = 0
    sa, sb = ea.stats(), eb.stats()
    assert sa == sb
    for k, v in st.items():
        assert sa[k] == v, k
    # (the device adds the envs' returns in a fixed tree, the loop above env by env: equal up to the rounding of a sum of n terms)
    assert np.allclose(sa["return_sum"], ret_sum, rtol=0, atol=1e-9)
    # truncation, the reset pass and the other layout's descriptor row all happened
    assert st["truncations"] >= 2 * n and int(orc.records[:, soa.W_EPISODE].min()) >= 2 and layouts_seen == {0, 1}
    ea.close(), eb.close()
    assert seen == {expect}, f"lean variants taken: {[hex(v) for v in seen]}, expected {hex(expect)}"


@pytest.mark.parametrize("n", [9, 1])
@pytest.mark.parametrize("agents,scheme,R,end_all,walk_touches", ROWS)
def test_every_instantiated_combination_against_oracle(agents, scheme, R, end_all, walk_touches, n):
    """the handle's walk_touches is what cz_load_recipes decided (the default book with up to two agents: 0; more than two agents: 1):
    the variant code carries it, so a row whose walk_touches the handle does not have is reported as a fallback here"""
    run_against_oracle(n, agents, scheme, R, end_all, code(R, end_all, walk_touches))
    RAN.add((agents, scheme, R, end_all, walk_touches, n))


@pytest.mark.parametrize("agents,scheme,R", [(2, 1, 2), (4, 3, 4), (1, 1, 1)])
def test_other_combinations_fall_back_to_the_lean_kernel(agents, scheme, R):
    assert not any(r[:3] == (agents, scheme, R) for r in ROWS)
    run_against_oracle(9, agents, scheme, R, 0, 0)


def test_switch_keeps_the_lean_kernel():
    """CZ_LEAN_CFG=0 (A/B runs): the same handle takes k_step_lean"""
    os.environ["CZ_LEAN_CFG"] = "0"
    try:
        run_against_oracle(9, 2, 3, 2, 0, 0)
    finally:
        del os.environ["CZ_LEAN_CFG"]


def replay(gs, enabled):
    """the golden episodes of one set through cz_step_device; -> per-step (records, obs, rewards, term, trunc), stats, variants"""
    eps = gs.episodes
    with lean(enabled):
        h, rids, _ = handle_for_set(gs)
    n, A, F = len(eps), eps[0].dims.A, eps[0].dims.F
    h.reset(np.arange(n), rids, want_obs=False)
    d_act, d_obs = h.dev_alloc(n * A * 4), h.dev_alloc(n * A * F * 8)
    d_rew, d_term, d_trunc = h.dev_alloc(n * A * 8), h.dev_alloc(n * A), h.dev_alloc(n * A)
    out, seen = [], set()
    for t in range(max(len(ep.actions) for ep in eps)):
        acts = np.zeros((n, A), dtype=np.int32)
        for i, ep in enumerate(eps):
            if t < len(ep.actions):
                acts[i] = ep.actions[t]
        h.h2d(d_act, acts)
        h.ck(h.L.cz_step_device(h.h, C.c_void_p(d_act), C.c_void_p(d_obs), C.c_void_p(d_rew), C.c_void_p(d_term), C.c_void_p(d_trunc)))
        seen.add(variant(h.h))
        out.append((h.get_state(), h.d2h(d_obs, (n, A, F), np.float64), h.d2h(d_rew, (n, A), np.float64),
                    h.d2h(d_term, (n, A), np.uint8), h.d2h(d_trunc, (n, A), np.uint8)))
    st = h.stats()
    h.close()
    return out, st, seen


# (under "all dishes" no golden episode delivers both dishes: its deliveries are rewarded, nothing terminates)
@pytest.mark.parametrize("name,expect,terminates", [("cfg2_coop_2agents", code(2, 0, 0), True), ("cfg2_all_dishes", code(2, 1, 0), False),
                                                    ("cfg1_coop_1agent", code(1, 0, 0), True)])
def test_golden_episodes_with_delivered_dishes(name, expect, terminates):
    gs = GoldenSet(name)
    assert any(ep.terms.any() for ep in gs.episodes) == terminates, f"{name}: golden episodes that end by a delivered dish"
    assert any((np.asarray(ep.rewards) > 0).any() for ep in gs.episodes), f"{name}: no golden step rewards a recipe"
    a, st_a, va = replay(gs, True)
    b, st_b, vb = replay(gs, False)
    assert va == {expect} and vb == {-1}, (va, vb)
    assert st_a == st_b
    for t, (x, y) in enumerate(zip(a, b)):
        for k, (u, v) in enumerate(zip(x, y)):
            assert u.tobytes() == v.tobytes(), f"{name} step {t}: output {k} differs between the lean and the generic kernel"
    for t, (rec, obs, rew, term, trunc) in enumerate(a):
        for i, ep in enumerate(gs.episodes):
            if t >= len(ep.actions):
                continue
            ctx = f"{name} ep{i} step {t}"
            assert np.array_equal(strip_golden(rec[i]), strip_golden(ep.states[t + 1])), f"{ctx}: state"
            assert np.array_equal(bits(rew[i]), bits(ep.rewards[t])), f"{ctx}: reward"
            assert np.array_equal(term[i], ep.terms[t]) and np.array_equal(trunc[i], ep.truncs[t]), f"{ctx}: flags"
            assert np.array_equal(bits(obs[i]), bits(ep.obs[t + 1])), f"{ctx}: obs"


def test_every_instantiated_combination_ran():
    """runs last: every row of CZ_LEAN_CFGS was taken by a handle at both batch sizes - none skipped, none left out of the list"""
    assert len(ROWS) == len(set(ROWS)) and 1 <= len(ROWS) <= 16
    assert sorted(set(r[:5] for r in RAN)) == sorted(ROWS) and len(RAN) == 2 * len(ROWS)
    # R = 1..4 with the end condition both ways, walk_touches both ways
    assert {(r[2], r[3]) for r in ROWS} >= {(R, ea) for R in (1, 2, 3, 4) for ea in (0, 1)}
    assert {r[4] for r in ROWS} == {0, 1}
