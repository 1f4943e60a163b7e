"""A submitted FAV batch's verdicts survive every other call on its job.

Job 0 is shared: the per-call entry points, the pairing and curve calls, grouped aggregation, the G1 table, the
signing-root kernels, blob and cell KZG all run on its streams and scratch slots, and a batch submitted through the
job API may sit there between its submit and its finish.  Every cell of the tables below leaves a batch pending
(job_isolation_inputs.pending: 10 items of 8 keys, item 3 invalid), makes one call -- or all of them -- on the same
context (job_isolation_inputs.CALLS), and asserts three things: the batch check still says False, the interleaved
call returns its expected value, and the verdict bytes after the finish equal, bit for bit, those of the same batch,
seed and route with nothing in between (which must themselves be the built-in expected verdicts).

Routes to a verdict:
  R1  submit(0), job_partial, job_check -> finish           R3  submit(0), job_check_comm -> finish (communicator)
  R2  submit(0), job_check_own -> finish                    R4  partial(), check_partials, finish()  (indexed only)
R1 and R2 run on the communicator context too: its submit leaves the job's own check for later (read_own), whichever
call the caller reads the verdict with.  Position "a" puts the call between the submit and the check, "b" between
the check and the finish.

test_failing_shard_under_a_communicator_is_not_accepted_after_a_passing_product is the sequence that accepted an
invalid signature: read_own used to check whatever S_FPART held at the finish, and a passing per-call product there
made the failing shard keep every status."""
import contextlib

import numpy as np
import pytest

import job_isolation_inputs as J
import kzg_inputs as K
from test_gpu_comm import DictStore

pytestmark = pytest.mark.gpu

BAD3 = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
assert J.pending("indexed", "bad3").expect == BAD3
POISON = 0xEE


class Env:
    """One context with what the calls need resident on it: the registry of 128 keys, the committee table, the
    blob KZG setup (verification only), the cell setup (made again whenever a call has replaced the G1 table), and
    the pending batches in HBM."""

    def __init__(self, ctx):
        from bls_mi355x import _native, batch, curve, kzg, kzg_cells
        from bls_mi355x import bls as shim

        shim.use_mi355x()
        shim.bls_active = True
        self.ctx, self.native, self.batch, self.curve, self.shim = ctx, _native, batch, curve, shim
        self.kzg_cells = kzg_cells
        self.registry = batch.Registry(ctx)
        assert self.registry.load(b"".join(J.pubkeys())).all()
        self.committees = batch.Committees(ctx).load(J.committee_lists())
        self.kzg = kzg.KzgSetup.verify_only(K.trusted_setup()[2][1], ctx=ctx)
        self._cells, self._cells_gen = None, None
        self._resident, self._control = {}, {}

    @contextlib.contextmanager
    def as_default(self):
        """the shim and the curve objects work on the default context: this one, for the duration"""
        saved = self.native._ctx
        self.native._ctx = self.ctx
        try:
            yield
        finally:
            self.native._ctx = saved

    def cells(self):
        gen = int(self.ctx.lib.bls_g1_table_generation(self.ctx.h))
        if self._cells is None or gen != self._cells_gen:
            _, mono, g2 = K.trusted_setup()
            with self.as_default():
                self._cells = self.kzg_cells.CellSetup(self.ctx, mono[:64], g2[64])
            self._cells_gen = int(self.ctx.lib.bls_g1_table_generation(self.ctx.h))
        return self._cells

    def resident(self, form, variant):
        key = (form, variant)
        if key not in self._resident:
            self._resident[key] = J.pending(form, variant).resident(self.batch, self.ctx, self.committees)
        return self._resident[key]

    def call(self, name):
        """(result, expected) of one interleaved call"""
        with self.as_default():
            return J.CALLS[name](self)

    def free(self):
        for rb in self._resident.values():
            rb.free()
        self._resident = {}


@pytest.fixture(scope="module")
def plain():
    from bls_mi355x import _native, curve

    curve.use_g1_table(None)
    env = Env(_native.context())
    yield env
    env.free()


@pytest.fixture(scope="module")
def comm():
    """a context of its own with a world-1 communicator, set up and torn down as test_gpu_comm.py does"""
    from bls_mi355x import _native, dist

    ctx = _native.Context()
    env = Env(ctx)
    dist.init_comm(ctx, 0, 1, DictStore())
    try:
        yield env
    finally:
        env.free()
        dist.destroy_comm(ctx)
        ctx.close()


@pytest.fixture
def envs(plain, comm):
    return {"plain": plain, "comm": comm}.__getitem__


def run_route(env, rb, route, a=None, b=None, job=0, finish_ok=None):
    """One pass of the batch over the route with the callables a / b at the two positions; finish_ok overrides
    what the finish is told.  Returns (the check's verdict, the verdict bytes)."""
    c = env.ctx
    poison = np.full(rb.B, POISON, dtype=np.uint8)
    out = rb.outs[job]
    c.check(c.lib.bls_h2d(c.h, out.ptr, poison.ctypes.data, rb.B))
    if route == "R4":
        assert job == 0
        part = rb.partial(J.SEED)
        if a:
            a()
        ok = rb.check_partials(part)
        if b:
            b()
        rb.finish(ok if finish_ok is None else finish_ok)
    else:
        rb.submit(job, J.SEED)
        if a:
            a()
        if route == "R1":
            ok = rb.job_check(job, rb.job_partial(job))
        elif route == "R2":
            ok = rb.job_check_own(job)
        else:
            assert route == "R3"
            ok = rb.job_check_comm(job)
        if b:
            b()
        rb.job_finish(job, ok if finish_ok is None else finish_ok)
    return ok, [int(v) for v in out.to_host()]  # the copy waits for every job's stream


def control(env, route, form, variant, finish_ok=None):
    """the same batch, seed and route with nothing in between: computed once, and it is the built-in expectation"""
    key = (route, form, variant, finish_ok)
    if key not in env._control:
        ok, v = run_route(env, env.resident(form, variant), route, finish_ok=finish_ok)
        p = J.pending(form, variant)
        assert ok is (variant == "good") and v == p.expect, (key, ok, v)
        env._control[key] = (ok, v)
    return env._control[key]


def at(pos, step):
    return {"a": step, "b": None} if pos == "a" else {"a": None, "b": step}


ROUTES = [("plain", "R1"), ("plain", "R2"), ("plain", "R4"), ("comm", "R1"), ("comm", "R2"), ("comm", "R3")]
ROUTE_IDS = ["%s-%s" % r for r in ROUTES]
OWN_ROUTES = [("plain", "R2"), ("comm", "R3")]
OWN_IDS = ["%s-%s" % r for r in OWN_ROUTES]


# ---- 1. indexed bad3: every route x every non-replacing call x both positions ---------------------------------------
@pytest.mark.parametrize("pos", ["a", "b"])
@pytest.mark.parametrize("name", list(J.CALLS))
@pytest.mark.parametrize("kind,route", ROUTES, ids=ROUTE_IDS)
def test_one_call_leaves_the_pending_batch_alone(envs, kind, route, name, pos):
    env = envs(kind)
    want_ok, want_v = control(env, route, "indexed", "bad3")
    seen = []
    ok, v = run_route(env, env.resident("indexed", "bad3"), route, **at(pos, lambda: seen.append(env.call(name))))
    assert ok is False and want_ok is False
    (got, want), = seen
    assert got == want, name
    assert v == want_v == BAD3


# ---- 2. indexed good, finish(batch_ok = 0): the failure the caller reports lies in another shard --------------------
@pytest.mark.parametrize("pos", ["a", "b"])
@pytest.mark.parametrize("name", ["verify_failing", "pairing_check_failing"])
@pytest.mark.parametrize("kind,route", ROUTES, ids=ROUTE_IDS)
def test_a_failing_call_does_not_make_a_good_shard_bisect_wrong(envs, kind, route, name, pos):
    env = envs(kind)
    assert control(env, route, "indexed", "good", finish_ok=False) == (True, [1] * J.B)
    seen = []
    ok, v = run_route(env, env.resident("indexed", "good"), route, finish_ok=False,
                      **at(pos, lambda: seen.append(env.call(name))))
    assert ok is True
    assert seen == [(False, False)]
    assert v == [1] * J.B


# ---- 3. the other forms: all non-replacing calls in one sequence -----------------------------------------------------
def all_calls(env, seen):
    for name in J.CALLS:
        seen.append((name,) + env.call(name))


@pytest.mark.parametrize("pos", ["a", "b"])
@pytest.mark.parametrize("form", ["shared", "bits", "keys"])
@pytest.mark.parametrize("kind,route", OWN_ROUTES, ids=OWN_IDS)
def test_every_call_in_turn_leaves_the_other_forms_alone(envs, kind, route, form, pos):
    env = envs(kind)
    want_ok, want_v = control(env, route, form, "bad3")
    seen = []
    ok, v = run_route(env, env.resident(form, "bad3"), route, **at(pos, lambda: all_calls(env, seen)))
    assert ok is False and want_ok is False
    assert [n for n, _, _ in seen] == list(J.CALLS)
    assert [n for n, got, want in seen if got != want] == []
    assert v == want_v == BAD3


def test_the_bits_batch_has_items_in_complement_mode(plain):
    rb = plain.resident("bits", "bad3")
    rb.run_pipelined([J.SEED])
    points, complement_items = plain.batch.gather_work(plain.ctx)
    assert complement_items >= 2 and list(rb.verdicts()) == [bool(x) for x in BAD3]


# ---- 4. calls that replace the slot's batch, or the tables it read --------------------------------------------------
REPLACED = [1, 1, 1, 1, 1, 1, 0, 1, 1, 1]


@pytest.mark.parametrize("form", J.REPLACING)
@pytest.mark.parametrize("kind,route", OWN_ROUTES, ids=OWN_IDS)
def test_a_host_batch_after_the_check_replaces_the_batch_the_finish_judges(envs, kind, route, form):
    """include/blsmi355x.h: another batch prepared on the job since its submit voids the own verdict, and a failing
    finish bisects from the root -- the batch that is there, so its verdicts (item 6), not the submitted one's"""
    env = envs(kind)
    rep = J.replacing(form)
    assert rep.expect == REPLACED
    seen = []
    ok, v = run_route(env, env.resident("indexed", "bad3"), route, finish_ok=False,
                      b=lambda: seen.append(rep.host_call(env.batch, env.ctx, env.committees)))
    assert ok is False
    assert seen == [REPLACED]
    assert v == REPLACED


@pytest.mark.parametrize("form", J.REPLACING)
def test_a_host_batch_before_the_check_voids_the_own_verdict(plain, form):
    """... and bls_fav_job_check_own is then BLS_E_ARG"""
    env, rep = plain, J.replacing(form)
    rb = env.resident("indexed", "bad3")
    rb.submit(0, J.SEED)
    assert rep.host_call(env.batch, env.ctx, env.committees) == REPLACED
    with pytest.raises(env.native.NativeError, match="-2"):
        rb.job_check_own(0)
    rb.job_finish(0, False)
    assert [int(x) for x in rb.outs[0].to_host()] == REPLACED


@pytest.mark.parametrize("pos", ["a", "b"])
@pytest.mark.parametrize("kind,route", OWN_ROUTES, ids=OWN_IDS)
def test_reloading_the_committee_table_keeps_a_pending_bits_batchs_verdicts(envs, kind, route, pos):
    """bls_committees_load waits for the device first: the pending batch has gathered its keys from the old table"""
    env = envs(kind)
    want_ok, want_v = control(env, route, "bits", "bad3")
    step = lambda: env.committees.load(J.committee_lists())
    ok, v = run_route(env, env.resident("bits", "bad3"), route, **at(pos, step))
    assert ok is False and want_ok is False
    assert len(env.committees) == J.N_COMM
    assert v == want_v == BAD3


# ---- 5. neighbour jobs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,route", OWN_ROUTES, ids=OWN_IDS)
def test_per_call_work_touches_no_other_jobs_slots(envs, kind, route):
    env = envs(kind)
    bad, good = env.resident("indexed", "bad3"), env.resident("indexed", "good")
    c = env.ctx
    poison = np.full(J.B, POISON, dtype=np.uint8)
    c.check(c.lib.bls_h2d(c.h, bad.outs[1].ptr, poison.ctypes.data, J.B))
    c.check(c.lib.bls_h2d(c.h, good.outs[0].ptr, poison.ctypes.data, J.B))
    bad.submit(1, J.SEED)
    good.submit(0, J.SEED)
    seen = []
    all_calls(env, seen)
    assert [n for n, got, want in seen if got != want] == []
    check = (lambda rb, job: rb.job_check_own(job)) if route == "R2" else (lambda rb, job: rb.job_check_comm(job))
    ok1, ok0 = check(bad, 1), check(good, 0)
    assert (ok1, ok0) == (False, True)
    bad.job_finish(1, ok1)
    good.job_finish(0, ok0)
    assert [int(x) for x in bad.outs[1].to_host()] == BAD3
    assert [int(x) for x in good.outs[0].to_host()] == [1] * J.B


# ---- the sequence that accepted an invalid signature ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["verify", "pairing_check", "aggregate_verify"])
def test_failing_shard_under_a_communicator_is_not_accepted_after_a_passing_product(comm, name):
    """A bad batch on job 0 under a world-1 communicator, a passing per-call check, finish(0, 0): item 3 is
    rejected.  pairing_check and AggregateVerify leave their passing product in S_FPART, where the job's own check
    used to look for the batch's."""
    rb = comm.resident("indexed", "bad3")
    c = comm.ctx
    poison = np.full(J.B, POISON, dtype=np.uint8)
    c.check(c.lib.bls_h2d(c.h, rb.outs[0].ptr, poison.ctypes.data, J.B))
    rb.submit(0, J.SEED)
    assert comm.call(name) == (True, True)
    assert rb.job_check_comm(0) is False
    rb.job_finish(0, False)
    assert [int(x) for x in rb.outs[0].to_host()] == BAD3
