"""The fork / issue / join order of the backward's weight-gradient side stream (shot_vae_amd/sidestream.py), on recorded device
primitives: no GPU, no library.  The expected sequences are those of the scheduler's measured rules: the paired main-stream launch is
issued FIRST, a flag fork needs a launch that carries the signal, the first pair behind a fused backward forks by event."""
import contextlib
from types import SimpleNamespace

import pytest

import shot_vae_amd.engine as E
from shot_vae_amd.sidestream import WgradSideStream

MAIN, SIDE = SimpleNamespace(cuda_stream=11), SimpleNamespace(cuda_stream=22)
FLAG = (0xF1A6, 7)


class Recorder(WgradSideStream):
    """the scheduler with every device primitive replaced by an entry in self.ev"""

    def __init__(self, engine, capturing=False):
        super().__init__(engine)
        self.ev, self.on, self.capturing = [], "main", capturing
        self.streams[MAIN.cuda_stream] = SIDE              # (the pool would create a torch.cuda.Stream here)

    def _current_stream(self):
        return MAIN

    @contextlib.contextmanager
    def _on(self, side):
        assert side is SIDE
        self.on = "side"
        try:
            yield
        finally:
            self.on = "main"

    def _fork(self, cur, side, light):
        self.ev.append(("fork", cur.cuda_stream, side.cuda_stream, light))

    def _flag_next(self, cur):
        self.ev.append(("flag_next", cur.cuda_stream))
        return FLAG

    def _wait_flag(self, side, flag, value):
        self.ev.append(("wait_flag", side.cuda_stream, flag, value))

    def _wait_stream(self, cur, side):
        self.ev.append(("wait_stream", cur.cuda_stream, side.cuda_stream))

    def _capturing(self):
        return self.capturing

    def _synchronize(self):
        self.ev.append(("sync",))


def make(capturing=False, **switches):
    eng = SimpleNamespace(wgrad_side_stream=True, prof_tags=None, flag_fork=True, light_fork=True, fork_every=1,
                          event_fork_after_fused=True, _flag_forks_verified=True)
    eng.__dict__.update(switches)
    s = Recorder(eng, capturing)
    eng._wgrad = lambda *job: s.ev.append(("wgrad", s.on, job[5]))
    return s


def job(n=1):
    """(g, x, pro, dy, dw_ptr, tag, groups, budget) as Engine._wgrad takes it; x / dy are what the scheduler keeps alive"""
    return ("g%d" % n, "x%d" % n, None, "dy%d" % n, 0, "w%d" % n, 1, 0)


def then(s, n=1, take=True, taken=None):
    def fn():
        s.ev.append(("then%d" % n,))
        if take:
            got = (s.take_start_signal(), s.take_start_signal())
            if taken is not None:
                taken.append(got)
        return "out%d" % n
    return fn


FORK = ("fork", 11, 22, True)
FLAG_PAIR = [("flag_next", 11), ("then1",), ("wait_flag", 22, FLAG[0], FLAG[1]), ("wgrad", "side", "w1")]


@pytest.fixture(autouse=True)
def not_serialised(monkeypatch):
    monkeypatch.setattr(E, "_dispatch_serialised", lambda: False)


@pytest.mark.parametrize("why", ["switch", "prof_tags", "capturing"])
def test_not_enabled_runs_the_weight_gradient_on_the_main_stream(why):
    s = make(capturing=why == "capturing", **({"wgrad_side_stream": False} if why == "switch" else
                                              {"prof_tags": {}} if why == "prof_tags" else {}))
    assert not s.enabled()
    assert s.submit(job(), then(s)) == "out1"
    assert s.ev == [("wgrad", "main", "w1"), ("then1",)]
    assert not s.pending and not s.keep and s.start_signal is None
    assert s.submit(job()) is None
    s.join()
    s.flush()
    assert s.ev == [("wgrad", "main", "w1"), ("then1",), ("wgrad", "main", "w1")]


def test_flag_fork():
    s, taken = make(), []
    assert s.enabled()
    assert s.submit(job(), then(s, taken=taken)) == "out1"
    assert s.ev == FLAG_PAIR
    assert taken == [(FLAG, None)]                       # handed out once
    assert s.keep == {11: [("x1", "dy1")]} and s.pending == [] and s.start_signal is None
    assert s.side_of(MAIN) is SIDE and s.side_of(SimpleNamespace(cuda_stream=33)) is None


def test_flag_fork_falls_back_to_an_event_when_no_launch_took_the_signal():
    s = make(light_fork=False)
    assert s.submit(job(), then(s, take=False)) == "out1"
    assert s.ev == [("flag_next", 11), ("then1",), ("fork", 11, 22, False), ("wgrad", "side", "w1")]
    assert s.start_signal is None and s.take_start_signal() is None


def test_a_failing_then_disarms_the_signal_and_abort_clears_the_rest():
    s = make()
    s.submit(job(1), then(s, 1))                          # (a finished pair: its operands are kept)
    s.ev.clear()

    def boom():
        s.ev.append(("then2",))
        raise RuntimeError("launch failed")
    with pytest.raises(RuntimeError, match="launch failed"):
        s.submit(job(2), boom)
    assert s.ev == [("flag_next", 11), ("then2",)]        # nothing was issued on the side stream
    assert s.start_signal is None
    assert s.pending == [job(2)] and s.keep == {11: [("x1", "dy1")]}
    s.note_fused()
    s.abort()
    assert s.ev[-1] == ("sync",)
    assert s.pending == [] and s.keep == {} and s.start_signal is None and s.fused_since_fork is False


def test_the_first_pair_behind_a_fused_backward_forks_by_event():
    s = make()
    s.note_fused()
    assert s.submit(job(), then(s)) == "out1"
    assert s.ev == [FORK, ("then1",), ("wgrad", "side", "w1")]
    s.ev.clear()
    s.submit(job(), then(s))                              # the next pair forks by flag again
    assert s.ev == FLAG_PAIR
    s = make(event_fork_after_fused=False)
    s.note_fused()
    s.submit(job(), then(s))
    assert s.ev == FLAG_PAIR and s.fused_since_fork is False


def test_event_fork_without_a_then_and_under_serialised_dispatch(monkeypatch):
    s = make()
    assert s.submit(job()) is None
    assert s.ev == [FORK, ("wgrad", "side", "w1")]
    monkeypatch.setattr(E, "_dispatch_serialised", lambda: True)
    s = make()
    assert s.submit(job(), then(s)) == "out1"
    assert s.ev == [FORK, ("then1",), ("wgrad", "side", "w1")]


def test_fork_every_two_shares_one_fork():
    s = make(fork_every=2)
    assert s.submit(job(1), then(s, 1)) == "out1"
    assert s.ev == [("then1",)] and s.pending == [job(1)] and not s.keep
    assert s.submit(job(2), then(s, 2)) == "out2"
    assert s.ev == [("then1",), FORK, ("then2",), ("wgrad", "side", "w1"), ("wgrad", "side", "w2")]
    assert s.pending == [] and s.keep == {11: [("x1", "dy1"), ("x2", "dy2")]}


def test_flush_and_join_with_event_forks():
    s = make(fork_every=2, flag_fork=False)
    s.flush()
    assert s.ev == []
    s.submit(job())
    s.flush()
    assert s.ev == [FORK, ("wgrad", "side", "w1")] and s.pending == []
    s.ev.clear()
    s.submit(job(2))
    s.join()
    assert s.ev == [FORK, ("wgrad", "side", "w2"), ("wait_stream", 11, 22)]
    assert s.keep == {} and s.pending == []
    s = make(wgrad_side_stream=False)
    s.join()
    assert s.ev == []
