"""No device: tests/stream_hold.py against stand-ins of torch.cuda.Stream / torch.cuda.Event with the same four methods (and the same nesting:
wait_stream = wait_event(record_event()), record_event = event.record(stream)), patched in place of the torch ones."""
import pytest

import stream_hold as H


def make_api():
    """Fresh stand-in classes per test, and the log of what reached the 'device': ("record", stream), ("wait", stream), ("delay", stream, ms)."""
    log, current = [], []

    class Event:
        def record(self, stream=None):
            log.append(("record", (current[-1] if stream is None else stream).cuda_stream))

        def wait(self, stream):
            log.append(("wait", stream.cuda_stream))

    class Stream:
        def __init__(self, handle):
            self.cuda_stream = handle

        def wait_event(self, event):
            event.wait(self)

        def wait_stream(self, stream):
            self.wait_event(stream.record_event())

        def record_event(self, event=None):
            if event is None:
                event = Event()
            event.record(self)
            return event

    class Api:
        pass
    api = Api()
    api.Stream, api.Event, api.log, api.current = Stream, Event, log, current
    api.current_stream = lambda: current[-1]
    api.enqueue_delay = lambda stream, ms: log.append(("delay", stream.cuda_stream, ms))
    return api


@pytest.fixture
def rig():
    api = make_api()
    caller, side, pre = api.Stream(0), api.Stream(0x10), api.Stream(0x20)
    api.current.append(caller)
    roles = H.RoleMap().add("caller", caller).add("side:b", side).add("pre:b", pre)
    return api, roles, caller, side, pre


def fork_join(api, caller, side):
    """ScaleEngine._fork / _join, and a wait_stream each way."""
    fork, join = api.Event(), api.Event()
    fork.record()
    side.wait_event(fork)
    join.record(side)
    caller.wait_event(join)
    side.wait_stream(caller)
    caller.wait_stream(side)
    side.record_event()


def test_one_count_per_outermost_call(rig):
    api, roles, caller, side, _ = rig
    with H.hold(None, roles, 0, api) as ledger:
        fork_join(api, caller, side)
    assert dict(ledger.counts) == {("caller", "record"): 1, ("side:b", "wait_event"): 1, ("side:b", "record"): 1, ("caller", "wait_event"): 1,
                                   ("side:b", "wait_stream"): 1, ("caller", "wait_stream"): 1, ("side:b", "record_event"): 1}
    assert not ledger.delays and not [e for e in api.log if e[0] == "delay"]
    assert "side:b" in ledger.table() and ledger.roles() == ["caller", "side:b"]
    # the calls themselves went through unchanged: wait_stream is still a record on the other stream and a wait on this one
    assert api.log[-5:] == [("record", 0), ("wait", 0x10), ("record", 0x10), ("wait", 0), ("record", 0x10)]


def test_delays_go_to_the_held_role_only_and_after_the_call(rig):
    api, roles, caller, side, pre = rig
    with H.hold("side:b", roles, 7.5, api) as ledger:
        assert api.log == [("delay", 0x10, 7.5)]           # one when the context opens, on the held stream
        fork_join(api, caller, side)
    assert api.log == [("delay", 0x10, 7.5),
                       ("record", 0),                                               # fork.record(): the caller acts, no delay
                       ("wait", 0x10), ("delay", 0x10, 7.5),                        # side.wait_event: the branch starts late
                       ("record", 0x10), ("delay", 0x10, 7.5),                      # join.record(side): what follows on side is late
                       ("wait", 0),                                                 # caller.wait_event: untouched
                       ("record", 0), ("wait", 0x10), ("delay", 0x10, 7.5),         # side.wait_stream(caller): ONE delay, behind the whole call
                       ("record", 0x10), ("wait", 0),                               # caller.wait_stream(side): side is not the acting stream
                       ("record", 0x10), ("delay", 0x10, 7.5)]                      # side.record_event()
    assert dict(ledger.delays) == {"side:b": 5}
    held = {k: v for k, v in ledger.counts.items() if k[0] == "side:b"}
    assert sum(held.values()) + 1 == ledger.delays["side:b"]
    with H.hold(None, roles, 0, api) as plain:
        fork_join(api, caller, side)
    assert plain.counts == ledger.counts                   # the held run and the reference run took the same path


def test_a_role_of_several_streams_and_a_zero_delay(rig):
    api, roles, caller, side, pre = rig
    side2 = api.Stream(0x30)
    roles.add("side:b", side2)
    with H.hold("side:b", roles, 0, api) as ledger:
        api.Event().record(side2)
        api.Event().record(stream=side)
    assert ledger.delays["side:b"] == 4 and ledger.counts[("side:b", "record")] == 2 and not [e for e in api.log if e[0] == "delay"]
    with pytest.raises(ValueError):
        roles.add("pre:b", side2)                          # one stream, two roles


def test_a_stream_outside_the_role_map_raises(rig):
    api, roles, caller, side, _ = rig
    stranger = api.Stream(0x99)
    for call in (lambda: api.Event().record(stranger), lambda: stranger.wait_event(api.Event()), lambda: caller.wait_stream(stranger),
                 lambda: stranger.wait_stream(caller), lambda: stranger.record_event()):
        with pytest.raises(H.UnknownStream):
            with H.hold(None, roles, 0, api):
                call()
    api.current.append(stranger)                            # ev.record() on a current stream nobody listed
    with pytest.raises(H.UnknownStream):
        with H.hold(None, roles, 0, api):
            api.Event().record()
    with pytest.raises(H.UnknownStream):
        with H.hold("pipe.small", roles, 1.0, api):        # a role no stream has
            pass


def test_the_patches_are_gone_after_the_context(rig):
    api, roles, caller, side, _ = rig
    before = {(c, n): c.__dict__[n] for c, n in ((api.Event, "record"), (api.Stream, "wait_event"), (api.Stream, "wait_stream"), (api.Stream, "record_event"))}
    with H.hold("caller", roles, 1.0, api):
        assert all(c.__dict__[n] is not f for (c, n), f in before.items())
    assert all(c.__dict__[n] is f for (c, n), f in before.items())
    with pytest.raises(RuntimeError, match="body"):
        with H.hold("caller", roles, 1.0, api):
            raise RuntimeError("body")
    assert all(c.__dict__[n] is f for (c, n), f in before.items())
    with pytest.raises(H.UnknownStream):
        with H.hold(None, roles, 0, api):
            api.Stream(0x77).record_event()
    assert all(c.__dict__[n] is f for (c, n), f in before.items())
    n = len(api.log)
    fork_join(api, caller, side)
    assert not [e for e in api.log[n:] if e[0] == "delay"]


def test_the_torch_methods_are_python_level_and_come_back():
    """The real classes: the four methods are plain functions in the classes' own __dict__ (a class-level setattr reaches every call site), and
    hold() puts the very same objects back.  No device is touched: nothing is called."""
    import torch
    names = ((torch.cuda.Event, "record"), (torch.cuda.Stream, "wait_event"), (torch.cuda.Stream, "wait_stream"), (torch.cuda.Stream, "record_event"))
    before = [c.__dict__[n] for c, n in names]
    assert all(callable(f) and hasattr(f, "__code__") for f in before)
    with H.hold(None, H.RoleMap(), 0):
        assert all(c.__dict__[n] is not f for (c, n), f in zip(names, before))
    assert all(c.__dict__[n] is f for (c, n), f in zip(names, before))
