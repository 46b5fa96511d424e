"""GPU: the forms of the step launch one after another on ONE handle - cz_rollout_policy_value, cz_rollout_f32, cz_rollout_policy,
cz_rollout_actions_f32, cz_step_device_f32, cz_step_device, cz_rollout_policy_value again - each from the same saved state.

Every other test compares one form with the oracle on a handle that does little else.  Here each call's outputs must equal, in bits,
what the same call writes on a fresh handle built from the same tables that has launched nothing else since set_state: nothing of one
call - a pointer, a packed set, a mode - may survive into the next.  All outputs of a handle are sentinel-filled before every call and
read back after it; each has a guard row, and an output the call did not name must come back untouched."""
import numpy as np
import pytest

from policy_common import ACT_SENT, NAN64, PolicyTraj, sets_for, weights
from value_common import ValueTraj, value_weights
from vec_common import CROWDED4, SENT64, SENTINEL, TWO, GuardedRows, env_of, instance, last_mode, tables_of

pytestmark = pytest.mark.gpu

T, MAX_STEPS, SEED, STEP0 = 3, 2, 411, 5
# (name, level, meta, agents, recipes, scheme, envs, vsets): the per-agent loop at its shortest useful length and its longest; neither
# env count is a multiple of the envs per workgroup.  sets_for(A): agent 0 on set 1, the last agent without a policy - that one has
# a value set (values under the action stream); of the others one shares the trunk, one takes a second hidden pass, one has none
CELLS = [("2agents-scheme3", "coop_test", "example", 2, TWO, "scheme3", 5, (1, 0)),
         ("4agents-scheme1", "crowded_6x5", "crowded_6x5", 4, CROWDED4, "scheme1", 7, (1, 1, None, 0))]
FUSED = ("rows", "act", "logits", "rew", "term", "trunc")


class Handle:
    """one handle over the cell's tables with two weight sets and two value heads, at the saved state, and every output buffer"""

    def __init__(self, tables, W, V, state):
        env = self.env = env_of(tables)
        env.load_policy(*W)
        env.load_value(*V)
        env.reset(return_obs=False)
        n, A, F = env.num_envs, env.num_agents, env.F
        self.tr = ValueTraj(env, T)
        self.rows1 = GuardedRows(env)
        self.one = dict(obs1=(env.alloc((n + 1, A, F), np.uint64), SENT64), rew1=(env.alloc((n + 1, A), np.uint64), NAN64),
                        term1=(env.alloc((n + 1, A), np.uint8), 0xA5), trunc1=(env.alloc((n + 1, A), np.uint8), 0xA5))
        self.acts_in, self.act1 = env.alloc((T, n, A), np.int32), env.alloc((n, A), np.int32)
        self.state = env.get_state() if state is None else state

    def run(self, call, named, acts=None):
        """restore the saved state, fill every output, make the call -> {output: what came back without its guard, "state": records}"""
        env, tr = self.env, self.tr
        env.set_state(self.state)
        tr.fill()
        self.rows1.fill()
        for b, sent in self.one.values():
            b.from_host(np.full(b.shape, sent, b.dtype))
        if acts is not None:
            self.acts_in.from_host(acts)
            self.act1.from_host(acts[0])
        call(self)
        env.sync()
        mode = last_mode(env)
        out = tr.get()                                             # (asserts the guard rows of the seven fused outputs)
        out["rows1"] = self.rows1.rows()                           # (asserts its guard words)
        n = env.num_envs
        for k, (b, sent) in self.one.items():
            got = b.to_host()
            assert (got[n] == sent).all(), f"{k}: a store went past the last row"
            out[k] = got[:n]
        sentinels = dict({k: f[2] for k, f in tr.fillers.items()}, values=SENTINEL, rows1=SENTINEL, **{k: s for k, (_, s) in self.one.items()})
        for k, v in out.items():
            if k in named:
                assert (v != sentinels[k]).any(), f"{k}: the call named it and wrote nothing"
            else:
                assert (v == sentinels[k]).all(), f"{k}: the call did not name it, and it was written"
        out["state"] = env.get_state()
        return mode, out


def policy_value(vsets):
    def call(h):
        h.tr.vsets = vsets
        h.tr.launch(h.env, sets_for(h.env.num_agents), "sample", SEED, STEP0)
    call.__name__ = "rollout_policy_value"
    return call


def rollout_f32(h):
    b = h.tr.buf
    h.env.rollout_f32(T, SEED, STEP0, b["rows"], b["rew"], b["term"], b["trunc"])


def rollout_policy(h):
    PolicyTraj.launch(h.tr, h.env, sets_for(h.env.num_agents), "sample", SEED, STEP0)


def rollout_actions_f32(h):
    b = h.tr.buf
    h.env.rollout_actions_f32(h.acts_in, T, b["rows"], b["rew"], b["term"], b["trunc"])


def step_device_f32(h):
    b = h.one
    h.env.step_device_f32(h.act1, h.rows1, b["rew1"][0], b["term1"][0], b["trunc1"][0])


def step_device(h):
    b = h.one
    h.env.step_device(h.act1, b["obs1"][0], b["rew1"][0], b["term1"][0], b["trunc1"][0])


def same(ctx, a, b, keys):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), f"{ctx}: {k} differs in bits"


@pytest.mark.parametrize("cell", CELLS, ids=[c[0] for c in CELLS])
def test_seven_forms_on_one_handle_leave_what_each_leaves_alone(cell):
    _, level, meta, A, recipes, scheme, n, vsets = cell
    tables = tables_of(n, level, meta, A, recipes, scheme, MAX_STEPS, 8)
    W, V = weights(tables.F, tables.n_actions, 2, A, scale2=0.03), value_weights(2, A)
    H = Handle(tables, W, V, None)
    handles = [H]
    try:
        assert instance(H.env) == 0 and H.env.num_agents == A and H.env.policy_sets == 2 and H.env.value_sets == 2
        assert sets_for(A)[0] == 1 and sets_for(A)[-1] is None and vsets[-1] is not None
        fused_v, fused_p, fused_f = FUSED + ("values",), FUSED, ("rows", "rew", "term", "trunc")
        # (call, the outputs it names, the expected mode, whether it reads the actions call 3 wrote)
        sequence = [(policy_value(vsets), fused_v, 10, False), (rollout_f32, fused_f, 7, False), (rollout_policy, fused_p, 9, False),
                    (rollout_actions_f32, fused_f, 8, True), (step_device_f32, ("rows1", "rew1", "term1", "trunc1"), 6, True),
                    (step_device, ("obs1", "rew1", "term1", "trunc1"), 0, True), (policy_value(vsets), fused_v, 10, False)]
        results, acts = [], None
        for k, (call, named, want_mode, reads_actions) in enumerate(sequence, 1):
            ctx = f"call {k} ({call.__name__})"
            assert not reads_actions or acts is not None
            mode, got = H.run(call, named, acts if reads_actions else None)
            assert mode == want_mode, f"{ctx}: cz_diag_last_step_mode is {mode}, not {want_mode}"
            fresh = Handle(tables, W, V, H.state)
            handles.append(fresh)
            fresh_mode, alone = fresh.run(call, named, acts if reads_actions else None)
            assert fresh_mode == want_mode, f"{ctx} on a fresh handle: mode {fresh_mode}"
            same(f"{ctx} against the same call on a fresh handle", got, alone, got.keys())
            fresh.env.close()
            handles.pop()
            results.append(got)
            if k == 3:
                acts = got["act"].copy()
                assert (acts != ACT_SENT).all() and acts.shape == (T, n, A)
        r = results
        same("calls 1 and 7", r[0], r[6], r[0].keys())
        same("calls 3 and 4", r[2], r[3], ("rows", "rew", "term", "trunc", "state"))
        same("calls 3 and 1", r[2], r[0], [k for k in r[0] if k != "values"])
        # what makes the comparisons able to fail: the calls differ from one another where they should
        assert r[1]["rows"].tobytes() != r[2]["rows"].tobytes(), "the action stream and the policy give one trajectory: the case shows nothing"
        assert r[4]["rows1"].tobytes() == r[2]["rows"][0].tobytes(), "one float32 step over row 0 of the actions is row 0 of the trajectory"
        assert r[4]["state"].tobytes() == r[5]["state"].tobytes(), "the float32 and the float64 step leave one state"
        mask = np.array([v is not None for v in vsets])
        assert (r[0]["values"][:, :, mask] != SENTINEL).all() and (r[0]["values"][:, :, ~mask] == SENTINEL).all()
    finally:
        for h in handles:
            h.env.close()
