"""The backward's side stream: weight gradients are off the critical path, so they are issued on a stream of their own, forked off
the main stream in front of the data gradient they are paired with and joined at the end of the backward.  WgradSideStream owns
that schedule and all of its state; the switches that steer it (wgrad_side_stream, flag_fork, light_fork, fork_every,
event_fork_after_fused, prof_tags) stay on the Engine and are read through the engine reference at the moment of use."""
import ctypes as C

import torch

from . import _lib as L
from . import engine as _engine       # (_dispatch_serialised and the process-wide Engine switches, resolved at call time)


class WgradSideStream:
    def __init__(self, engine):
        self.engine = engine
        self.streams = {}             # main stream -> its side stream
        self.keep = {}                # main stream -> operands of the weight gradients in flight on its side stream
        self.pending = []             # weight gradients (the tuples Engine._wgrad takes) waiting for the next fork (fork_every)
        self.start_signal = None      # (flag, value) the next sv_igemm launch announces its start with (take_start_signal)
        self.fused_since_fork = False     # an sv_bwd3x3 launch has been issued since the last fork of the side stream

    # -- device primitives (one line each: a CPU test substitutes recorders) ---------------------------------------------------
    def _current_stream(self):
        return torch.cuda.current_stream()

    def _on(self, side):
        return torch.cuda.stream(side)

    def _fork(self, cur, side, light):
        L.call("sv_stream_fork", C.c_void_p(cur.cuda_stream), C.c_void_p(side.cuda_stream), int(light))

    def _flag_next(self, cur):
        flag, value = C.c_void_p(), C.c_uint32()
        L.call("sv_stream_flag_next", C.c_void_p(cur.cuda_stream), C.byref(flag), C.byref(value))
        return flag.value, value.value

    def _wait_flag(self, side, flag, value):
        L.call("sv_stream_wait_flag", C.c_void_p(side.cuda_stream), C.c_void_p(flag), C.c_uint32(value))

    def _wait_stream(self, cur, side):
        cur.wait_stream(side)

    def _capturing(self):
        return torch.cuda.is_current_stream_capturing()

    def _synchronize(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()

    def enabled(self):
        """the weight gradients run on the side stream now"""
        # (not under hipGraph capture: a captured step replays a hundred cross-stream edges slower than one stream --
        #  11.6 against 11.05 ms, measured -- and tensors freed during capture would need to outlive the side stream)
        return self.engine.wgrad_side_stream and self.engine.prof_tags is None and not self._capturing()

    def _pair(self):
        """(current stream, the side stream paired with it)"""
        cur = self._current_stream()
        return cur, self.streams.get(cur.cuda_stream) or self.streams.setdefault(cur.cuda_stream, torch.cuda.Stream())

    def side_of(self, stream):
        """the side stream paired with main stream `stream`, None if no weight gradient has run beside it yet"""
        return self.streams.get(stream.cuda_stream)

    def take_start_signal(self):
        """(flag, value) for the launch being built to announce its start with (sv_igemm_args::start_flag), or None.  Handed out
        once: the launch that takes it forks the side stream when it starts (see submit)."""
        signal, self.start_signal = self.start_signal, None
        return signal

    def note_fused(self):
        self.fused_since_fork = True

    def submit(self, job, then=None):
        """Enqueue the weight gradient `job` (the argument tuple of Engine._wgrad) behind everything issued so far, on the side
        stream: the dgrad -> BN-apply chain continues on the main stream without waiting for it (joined at the end of backward).
        `then`: a callable that issues the main-stream launch paired with this weight gradient (the layer's data gradient).
        It is issued FIRST, so that the main stream, the critical path, never waits for the host to finish the side stream's
        bookkeeping (tools/step_timeline.py showed ~8 us of idle main stream per pair), and it carries the fork: its first
        block stores a sequence number the side stream waits for (sv_igemm_args::start_flag, sv_stream_wait_flag) -- no event
        in the main stream's queue.  Without a `then` (or where dispatch is serialised: profilers) the fork is an event of the
        library's pool.  Either way the weight gradient depends only on what preceded the pair.  Returns `then`'s value."""
        e = self.engine
        if not self.enabled():
            e._wgrad(*job)
            return then() if then is not None else None
        cur, side = self._pair()
        # `fork_every` weight gradients share one fork: every fork is a marker in the main stream's queue that costs it ~6 us of
        # idle time in front of the next kernel (tools/probes/step_list.py: a gap before every data gradient)
        self.pending.append(job)
        if len(self.pending) < e.fork_every:
            return then() if then is not None else None
        # (the first pair behind fused-backward launches forks by event: the host runs ahead, the side stream's wait_flag_kernel for
        #  this pair would start as soon as the side stream is idle and spin on a CU THROUGH the fused launches in between -- 825 us in
        #  the trace -- and a fused launch whose waves fill the SIMDs' register files cannot share a CU with it: the workgroups the
        #  dispatcher had dealt to that CU's shader engine waited for a second round, 137 -> 236 us per launch of the residual form)
        after_fused, self.fused_since_fork = self.fused_since_fork and e.event_fork_after_fused, False
        if e.flag_fork and not after_fused and not _engine._dispatch_serialised() and then is not None and len(self.pending) == 1:
            # device-side fork: the paired main-stream launch (`then`, an sv_igemm) announces its own START through a flag word
            # (sv_igemm_args::start_flag) -- everything this weight gradient depends on has completed by then -- and the side
            # stream waits for the flag: no event, no marker in the main stream's queue
            flag, value = self.start_signal = self._flag_next(cur)
            try:
                out = then()
            finally:
                armed = self.take_start_signal()
            if armed is None:          # consumed by the launch
                self._wait_flag(side, flag, value)
            else:                      # (`then` launched nothing that could carry the signal: the ordinary fork, behind it)
                self._fork(cur, side, e.light_fork)
        else:
            # the fork is an event of the library's pool WITHOUT the system-scope fence of an ordinary event (sv_stream_fork,
            # Engine.light_fork): both streams are on this device
            self._fork(cur, side, e.light_fork)
            out = then() if then is not None else None
        self._issue(cur, side)
        return out

    def _issue(self, cur, side):
        with self._on(side):
            for job in self.pending:
                self.engine._wgrad(*job)
        # the operands stay referenced until the streams are joined at the end of backward (no record_stream bookkeeping
        # per tensor: two allocator calls per weight gradient on the host's critical path)
        self.keep.setdefault(cur.cuda_stream, []).extend((job[1], job[3]) for job in self.pending)
        self.pending = []

    def flush(self):
        """fork here, by event, and issue what is pending (fork_every > 1); nothing to do when nothing is pending"""
        if self.pending:
            cur, side = self._pair()
            self._fork(cur, side, self.engine.light_fork)
            self._issue(cur, side)

    def join(self):
        """End of a backward: the main stream waits for the side stream; the fail-closed checks of the flag fork."""
        if not self.enabled():
            return
        e = self.engine
        self.flush()
        cur, side = self._pair()
        self._wait_stream(cur, side)
        try:
            if e.flag_fork and not _engine._dispatch_serialised():
                # fail closed (sv_stream_wait_flag): the sticky time-out counter is host-mapped, the check is a memory read.  The
                # environment sniffing of _dispatch_serialised() cannot know every serialising tool, so the FIRST flag-forked
                # backward of an engine is verified with one synchronisation.  A wait that gave up THERE is recoverable: nothing
                # has consumed this backward's gradients yet (the optimizer step and the all-reduce come after it), so the engine
                # switches to event forks for good, clears the counter and reports THIS step invalid -- a caller that drops it
                # (zero_grad, next batch) continues on valid steps.
                if not e._flag_forks_verified:
                    self._synchronize()
                    _engine.Engine._flag_forks_verified = True
                    n = L.lib().sv_flag_timeouts()
                    if n:
                        _engine.Engine.flag_fork = False
                        e.flag_fork = False
                        L.call("sv_flag_timeouts_reset")
                        raise L.ShotVaeHipError(
                            "%d side-stream wait(s) for a data gradient's start signal timed out in the first backward of this "
                            "engine (kernel dispatch is serialised: profiler, debugger): the gradients of THIS backward are invalid "
                            "-- drop the step (zero_grad) -- and nothing has consumed them yet.  The engine now forks by events "
                            "(Engine.flag_fork = False); the following steps are valid." % n)
                # a LATER time-out is seen by this memory read only once the waiting kernel has run -- possibly a step late, after
                # sv_sgd / the all-reduce applied the corrupted gradients: that one is fatal (check_flag_timeouts says so)
                L.check_flag_timeouts("Engine.backward")
        finally:
            # the side stream's operands may be released now (also when the check raises): the main stream, on which the
            # allocator will hand their memory out again, is ordered behind everything the side stream did
            self.keep.pop(cur.cuda_stream, None)

    def abort(self):
        """After a failed backward: the operands kept alive for the side stream must not survive into the next step, nor may a
        half-made pair decide how the next one forks.  (The data-parallel bucket hook is NOT disarmed here yet.)"""
        self._synchronize()
        self.keep.clear()
        self.pending, self.start_signal, self.fused_since_fork = [], None, False
