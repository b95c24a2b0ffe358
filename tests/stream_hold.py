"""Holding one stream back (tests/test_stream_hold_ledger.py without a device, tests/test_gpu_stream_order.py with one).

The property: every hand-off between two streams is ordered by an event, a wait or a record_stream, never by the launches happening to land in
the right order.  ``hold(role, roles, delay)`` wraps the four Python-level synchronisation methods of torch/cuda/streams.py and follows ONE rule:
every synchronisation call in which a stream of the held role is the ACTING stream -- ``ev.record(S)``, ``S.wait_event(...)``, ``S.wait_stream(...)``,
``S.record_event(...)`` -- is followed by one delay enqueued on S, and one more delay goes on every stream of the role when the context opens.  Every
segment of the held role's work then starts late relative to every other stream; no wait is added or removed, no other stream is touched.  If the
held stream produces and a consumer did not wait, the consumer reads what was there before; if it reads and the next writer did not wait, it reads
what comes after.  With inputs that differ from clip to clip and scratch poisoned in between, both change the output bits.

The helper knows no kernels and no buffer names.  It keeps a ledger {(role, call kind): count} of the OUTERMOST calls of all roles
(``wait_stream`` is one call, not the ``record_event`` + ``record`` + ``wait_event`` it is made of) and raises ``UnknownStream`` when a call involves
a stream that is in no role: a stream added to the package later fails the test instead of going uncovered."""
import contextlib
from collections import Counter

KINDS = ("record", "wait_event", "wait_stream", "record_event")


class UnknownStream(LookupError):
    pass


class RoleMap(dict):
    """{stream.cuda_stream: role name}.  Several streams may share a role (a block's engines each have a side stream); one stream cannot have two
    roles -- torch hands streams out of a pool of 32 round robin, so engines made far apart can get the same one: make what a case uses in one go."""

    def __init__(self):
        super().__init__()
        self.streams = {}                                   # cuda_stream -> the stream object (the delay is enqueued through it)

    def add(self, role, stream):
        key = stream.cuda_stream
        if self.get(key, role) != role:
            raise ValueError(f"stream {key:#x} is {self[key]} and cannot also be {role}")
        self[key] = role
        self.streams[key] = stream
        return self

    def of(self, role):
        return [self.streams[k] for k, r in self.items() if r == role]

    def names(self):
        return sorted(set(self.values()))


class Ledger:
    def __init__(self):
        self.counts = Counter()                             # (role, kind) -> outermost calls
        self.delays = Counter()                             # role -> delays enqueued

    def roles(self):
        return sorted({r for r, _ in self.counts})

    def table(self):
        rows = [f"{'role':<24}" + "".join(f"{k:>13}" for k in KINDS) + f"{'delays':>9}"]
        for r in sorted(set(self.roles()) | set(self.delays)):
            rows.append(f"{r:<24}" + "".join(f"{self.counts[(r, k)]:>13}" for k in KINDS) + f"{self.delays[r]:>9}")
        return "\n".join(rows)


class TorchApi:
    """What ``hold`` patches and how it delays, for the real thing.  ``delay`` (milliseconds) becomes work through ``calibrate()``."""

    def __init__(self):
        import torch
        self.Stream, self.Event, self.current_stream = torch.cuda.Stream, torch.cuda.Event, torch.cuda.current_stream

    def prepare(self):
        calibrate()                                         # (its own events are recorded before the hooks are in place)

    def enqueue_delay(self, stream, delay):
        import torch
        with torch.cuda.stream(stream):
            calibrate().spin(delay)


@contextlib.contextmanager
def hold(role, roles, delay, api=None):
    """-> the Ledger of the calls made inside.  role None or delay 0: the same hooks, nothing enqueued (the reference run; a held role with
    delay 0 still counts the delays it would get)."""
    api = TorchApi() if api is None else api
    ledger, depth = Ledger(), [0]
    if delay and hasattr(api, "prepare"):
        api.prepare()
    saved = [(api.Event, "record"), (api.Stream, "wait_event"), (api.Stream, "wait_stream"), (api.Stream, "record_event")]
    saved = [(cls, name, cls.__dict__[name]) for cls, name in saved]

    def role_of(stream, what):
        key = stream.cuda_stream
        if key not in roles:
            raise UnknownStream(f"{what}: stream {key:#x} is in no role ({', '.join(roles.names()) if hasattr(roles, 'names') else sorted(set(roles.values()))})")
        return roles[key]

    def delay_on(stream, r):
        ledger.delays[r] += 1
        if delay:
            api.enqueue_delay(stream, delay)

    def wrap(kind, inner):
        def method(self, *args, **kw):
            if kind == "record":                            # ev.record(S = the current stream)
                acting = args[0] if args and args[0] is not None else kw.get("stream") or api.current_stream()
            else:
                acting = self
            r = role_of(acting, kind)
            if kind == "wait_stream":                       # (an event's stream was checked when it was recorded)
                role_of(args[0] if args else kw["stream"], kind)
            outermost = depth[0] == 0
            depth[0] += 1
            try:
                out = inner(self, *args, **kw)
            finally:
                depth[0] -= 1
            if outermost:
                ledger.counts[(r, kind)] += 1
                if r == role:
                    delay_on(acting, r)
            return out
        method.__name__ = kind
        return method

    try:
        for cls, name, inner in saved:
            setattr(cls, name, wrap(name, inner))
        if role is not None:
            held = roles.of(role)
            if not held:
                raise UnknownStream(f"no stream has the role {role}")
            for s in held:
                delay_on(s, role)
        yield ledger
    finally:
        for cls, name, inner in saved:
            setattr(cls, name, inner)


# ------------------------------------------------------------------------------------------------ the delay (with a device)
class _Delay:
    """``spin(ms)`` enqueues ``ms`` milliseconds of work on the current stream.  backend "sleep": torch.cuda._sleep, one wave that spins on the
    clock (it takes no CU from the other streams); backend "mm": a chain of small torch.mm on a private scratch, where _sleep is not steady."""

    def __init__(self, backend, units_per_ms, report):
        self.backend, self.units_per_ms, self.report, self._scratch = backend, units_per_ms, report, None

    def work(self, units):
        import torch
        if self.backend == "sleep":
            torch.cuda._sleep(int(units))
            return
        if self._scratch is None:
            a = torch.eye(1024, device="cuda") * 0.5
            self._scratch = (a, torch.empty_like(a), torch.empty_like(a))
        a, b, c = self._scratch
        for _ in range(max(1, int(units))):              # one unit: two products
            torch.mm(a, a, out=b)
            torch.mm(a, b, out=c)

    def spin(self, ms):
        self.work(ms * self.units_per_ms)


_DELAY = []


def _measure(delay, units, runs=3):
    import torch
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        delay.work(units)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def calibrate():
    """Once per session: units of work per millisecond from a pair of events, three times, and a check that twice the work takes twice as long.
    The rate comes from the FASTEST of the three, so that a requested delay is never shorter than asked."""
    if _DELAY:
        return _DELAY[0]
    import torch
    report = []
    for backend, units in (("sleep", 1 << 20), ("mm", 64)):
        d = _Delay(backend, 1.0, report)
        d.work(units)
        torch.cuda.synchronize()
        while min(_measure(d, units, 1)) < 2.0 and units < (1 << 40):
            units *= 4
        one, two = _measure(d, units), _measure(d, 2 * units)
        steady = max(one) / min(one) < 1.25 and 1.6 < min(two) / min(one) < 2.4
        report.append(f"{backend}: {units} units {[round(x, 3) for x in one]} ms, twice that {[round(x, 3) for x in two]} ms -> "
                      f"{'steady' if steady else 'NOT steady'}")
        if steady or backend == "mm":
            d.units_per_ms = units / min(one)
            report.append(f"delay backend: {backend}, {d.units_per_ms:.1f} units per ms")
            _DELAY.append(d)
            return d


def blocks(x, y, ms=3.0):
    """True when work on stream x keeps stream y from running (the two share a hardware queue): a spin of ``ms`` on x, a small fill on y around
    it, and the fill's completion timed on y.  A process has a few hardware queues and the streams are spread over them; a delay on x then holds
    y back too, which can hide a missing wait between the two and can never invent a difference."""
    import torch
    d = calibrate()
    with torch.cuda.stream(y):
        word = torch.zeros(1, device="cuda")

    def held_back():
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(y)
        with torch.cuda.stream(x):
            d.spin(ms)
        with torch.cuda.stream(y):
            word.fill_(1.0)
        b.record(y)
        torch.cuda.synchronize()
        return a.elapsed_time(b) > ms / 2
    return held_back() and held_back()                      # (a fill that another process's work delayed once is not a shared queue)


def time_ms(fn, before=None, runs=3):
    """(median, all) of ``runs`` event-timed calls of fn() on the current stream, after one warm-up call; before() runs in front of every call,
    untimed and followed by a synchronisation; fn synchronises before it returns."""
    import torch
    out = []
    for i in range(runs + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2], out
