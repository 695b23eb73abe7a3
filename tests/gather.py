"""Gathered calls (sgfhe_ctx_clone + csrc/coalescer.h) at a composition the test chooses.

tests/test_gpu_clone.py releases eight threads from a barrier and takes whatever the race gathers.  The coalescer's
own rules make the composition of a round controllable from outside:

 * a request of at most req_max gates that arrives while nobody is running leads alone and sets `running`;
 * everything that arrives during its run queues in `pending`, in arrival order;
 * the oldest queued request leads the next round and takes every queued request of its grouping key, in queue
   order, up to gates_max gates; what it leaves forms the round after, by the same rule.

So: a BLOCKER call on a clone of its own starts; follower threads, started beforehand and waiting on events, make
their calls a millisecond apart in the chosen order while it runs; when it returns the followers form exactly the
rounds the rules predict -- the first follower leads the first of them.  The blocker is a clone made slow on purpose
(one lane, chunks of 8, the throughput form: a chain of launches per 8 gates) and is sized from a measurement made
here: it is timed alone, and its batch grows until it lasts RATIO times the span from its start to the last
follower's release.  Its batch may exceed the req_max the case wants: it is admitted under a wider setting, and the
case's own knobs are set -- from another ctx, sgfhe_set_coalesce takes no lock the blocker holds -- once it runs.

run() ASSERTS the composition through sgfhe_coalesce_stats, reset before the run: exact calls, requests, gates and
max_requests.  A miss is neither a pass nor a skip: it is tried again with a blocker twice as long, at most twice
(host scheduling only: an unexpected exception, a HIP error or a timeout ends the run at once), then fails with the
figures seen.  Every attempt is appended to LOG and printed.

TEST INFRASTRUCTURE: a plain module (no conftest); nothing under sgfhe.jl_amd/ or bench.py imports it."""

import threading
import time

import numpy as np

STAGGER_S = 0.001       # between two followers' calls
LEAD_S = 0.005          # from the blocker's call to the case's knobs and the first follower
RATIO = 10              # the blocker alone lasts at least this many times the whole span
JOIN_S = 180            # a thread that is not back by then: the run is over, nothing is retried
ERR_HIP = -4
LOG = []                # dict(n, attempt, blocker_gates, blocker_ms, span_ms, stats, want) per attempt

_BATCH = {}             # blocker batch that sufficed, by ring size: where the next case starts


def inputs(params, batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, params.r, size=(batch, params.n), dtype=np.uint64),
            rng.integers(0, params.r, size=batch, dtype=np.uint64),
            rng.integers(0, params.r, size=(batch, params.n), dtype=np.uint64),
            rng.integers(0, params.r, size=batch, dtype=np.uint64))


class Job:
    """One follower: the call `work` on `eng` (an engine no other job uses), deterministic (key None) or as call
    number `call` of the draw stream keyed `key`; raw / rns2 as in Engine.bootstrap_batch, or `flags` verbatim
    through the C ABI (requests the binding cannot express)."""

    def __init__(self, eng, work, key=None, call=0, raw=False, rns2=False, flags=None):
        self.eng, self.work, self.key, self.call = eng, work, key, call
        self.raw, self.rns2, self.flags = raw, rns2, flags
        self.batch = len(work[1])

    def prepare(self, eng=None):
        """The flatten mode and the call counter of the job on `eng`: the calls before it are made, one gate each."""
        eng = eng or self.eng
        if self.key is None:
            eng.set_random_flatten(False)
            return
        eng.set_random_flatten(True, self.key)                       # call counter 0
        one = tuple(x[:1] for x in self.work)
        for _ in range(self.call):
            eng.bootstrap_batch(*one)

    def make(self, eng=None):
        eng = eng or self.eng
        if self.flags is None:
            return eng.bootstrap_batch(*self.work, raw=self.raw, rns2=self.rns2)
        import ctypes
        batch, (p1, q1, p2, q2), _keep = eng._lwe_args(*self.work)
        wide = bool(self.flags & 1)
        out = np.zeros((batch, 3, eng.params.n + 1) + ((2,) if wide else ()), dtype=np.uint64)
        eng._call("sgfhe_bootstrap_batch", p1, q1, p2, q2, batch, out.ctypes.data_as(ctypes.c_void_p), self.flags)
        return out


def alone(eng, jobs):
    """Every job's call made alone: on one clone of `eng`, gathering off, same flatten key and call number.  Errors
    come back as the exception.  Leaves gathering off (run() sets it)."""
    from sgfhe_jl_amd import SgfheError
    eng.set_coalesce(False)
    ref = eng.clone()
    try:
        out = []
        for j in jobs:
            j.prepare(ref)
            try:
                out.append(j.make(ref))
            except SgfheError as exc:
                out.append(exc)
        return out
    finally:
        ref.close()


class Blocker:
    """The clone whose call keeps `running` set while the followers queue."""

    def __init__(self, eng, params):
        self.params = params
        self.eng = eng.clone()
        self.eng.set_lanes(1)
        self.eng.set_chunk(8)
        self.eng.set_small_batch_max(0)
        self.batch = _BATCH.get(params.n, 8)
        self._work = None

    def work(self):
        if self._work is None or len(self._work[1]) != self.batch:
            self._work = inputs(self.params, self.batch, 4242)
        return self._work

    def timed(self):
        t0 = time.perf_counter()
        out = self.eng.bootstrap_batch(*self.work())
        return time.perf_counter() - t0, out

    def close(self):
        self.eng.close()


def _size_blocker(eng, bl, knobs, target_s):
    """Grow the blocker until, alone, it lasts target_s; returns (seconds, its result)."""
    for _ in range(8):
        eng.set_coalesce(True, max(bl.batch, knobs["req_max"]), max(bl.batch, knobs["gates_max"]), knobs["window_us"])
        dt, out = bl.timed()
        if dt >= target_s or bl.batch == 4096:
            break
        grown = int(bl.batch * min(16.0, 1.3 * target_s / dt)) + 8
        bl.batch = min(4096, (grown + 7) & ~7)
    assert dt >= target_s, "a blocker of %d gates lasts %.1f ms, %.1f ms wanted" % (bl.batch, dt * 1e3, target_s * 1e3)
    _BATCH[bl.params.n] = bl.batch
    return dt, out


def run(eng, bl, jobs, rounds, req_max=32, gates_max=256, window_us=300):
    """The jobs' calls, arriving in list order while the blocker runs.  `rounds`: the rounds the followers are to
    form, a list of lists of indices into `jobs` (None: results only, no composition asserted).  Returns the list of
    results, an SgfheError where the call failed.  Gathering is left on with the case's knobs: the caller restores
    the defaults (eng.set_coalesce(True)) in its `finally`."""
    from sgfhe_jl_amd import SgfheError
    knobs = dict(req_max=req_max, gates_max=gates_max, window_us=window_us)
    span = LEAD_S + STAGGER_S * len(jobs)
    target = RATIO * span
    want = None
    for attempt in range(3):
        for j in jobs:
            j.prepare()
        dt_alone, out_alone = _size_blocker(eng, bl, knobs, target)
        if rounds is not None:
            want = dict(calls=1 + len(rounds), requests=1 + sum(len(r) for r in rounds),
                        gates=bl.batch + sum(jobs[i].batch for r in rounds for i in r),
                        max_requests=max(len(r) for r in rounds))
        eng.coalesce_stats(reset=True)
        res, unexpected = [None] * len(jobs), []
        go = [threading.Event() for _ in jobs]
        started = threading.Event()
        bl_out, bl_end = [None], [None]

        def follower(i):
            go[i].wait()
            try:
                res[i] = jobs[i].make()
            except SgfheError as exc:
                res[i] = exc
            except BaseException as exc:                 # surfaced in the main thread
                unexpected.append(exc)

        def blocker():
            work = bl.work()
            started.set()
            try:
                bl_out[0] = bl.eng.bootstrap_batch(*work)
            except BaseException as exc:
                unexpected.append(exc)
            bl_end[0] = time.perf_counter()

        ts = [threading.Thread(target=follower, args=(i,)) for i in range(len(jobs))]
        tb = threading.Thread(target=blocker)
        for t in ts:
            t.start()
        tb.start()
        started.wait()
        t0 = time.perf_counter()
        time.sleep(LEAD_S)
        eng.set_coalesce(True, **knobs)                  # the case's knobs, while the blocker runs
        for g in go:
            g.set()
            time.sleep(STAGGER_S)
        t_last = time.perf_counter()
        for t in ts + [tb]:
            t.join(JOIN_S)
        hung = [t for t in ts + [tb] if t.is_alive()]
        assert not hung, "%d calls not back after %d s: nothing is retried" % (len(hung), JOIN_S)
        assert not unexpected, unexpected
        hip = [r for r in res if isinstance(r, SgfheError) and r.code == ERR_HIP]
        assert not hip, "HIP error in a gathered call, nothing is retried: %s" % hip
        assert bl_out[0].tobytes() == out_alone.tobytes(), "the blocker's own bytes changed"
        st = eng.coalesce_stats()
        rec = dict(n=bl.params.n, attempt=attempt, blocker_gates=bl.batch, blocker_ms=round(dt_alone * 1e3, 1),
                   span_ms=round((t_last - t0) * 1e3, 1), blocker_outlived_ms=round((bl_end[0] - t_last) * 1e3, 1),
                   stats=st, want=want)
        LOG.append(rec)
        print("gather:", rec)
        if want is None or st == want:
            return res
        target *= 2                                      # host scheduling: a longer blocker, the same case
    raise AssertionError("composition missed three times: wanted %r, last attempt %r" % (want, LOG[-1]))
