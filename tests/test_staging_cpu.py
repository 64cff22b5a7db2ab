"""isr2_amd/staging.py without a GPU: plain host buffers for slots and a stub event whose query() answer the test flips and whose
synchronize() calls are recorded.  Every wait carries a timeout, so a deadlock fails instead of hanging."""
import threading
import time

import pytest

from isr2_amd.staging import SKIP, ReadAhead, WriteBehind

TIMEOUT = 5.0


class Event:
    log = None                                                        # a list shared by the events of one test: the order of synchronize() calls

    def __init__(self, done=True, log=None, tag=None):
        self.done, self.log, self.tag, self.synced = done, log, tag, 0

    def query(self):
        return self.done

    def synchronize(self):
        self.synced += 1
        if self.log is not None:
            self.log.append(self.tag)
        self.done = True


def _within(fn):
    """Run fn() on a helper thread -> its result; fails when it has not returned within TIMEOUT (a deadlock), re-raises what it raised."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:                                    # noqa: BLE001
            box["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(TIMEOUT)
    assert not t.is_alive(), "deadlock: no return within the timeout"
    if "error" in box:
        raise box["error"]
    return box.get("value")


def _alive(name):
    return [t.name for t in threading.enumerate() if t.name.startswith(name)]


def _ended(name):
    t0 = time.monotonic()
    while _alive(name) and time.monotonic() - t0 < TIMEOUT:
        time.sleep(0.005)
    return not _alive(name)


def test_one_reader_yields_in_item_order_and_reuses_released_slots_only():
    slots = [bytearray(4) for _ in range(2)]
    held, seen_unreleased, used = set(), [], []

    def read(i, slot):
        if id(slot) in held:
            seen_unreleased.append(i)
        slot[0] = i
        used.append(id(slot))
        return i * 10

    def consume():
        make, got = iter(slots), []
        with ReadAhead(7, read, lambda: next(make), n_slots=2, name="t1-reader") as reads:
            for i, slot, payload in reads:
                held.add(id(slot))
                got.append((i, slot[0], payload))
                time.sleep(0.002)                                     # the reader is out of slots half of the time: it must wait
                held.discard(id(slot))
                reads.release(slot, Event(done=True))
        return got

    assert _within(consume) == [(i, i, 10 * i) for i in range(7)]
    assert not seen_unreleased
    assert len(used) == 7 and set(used) == {id(s) for s in slots}    # two slots carried seven items: each was reused
    assert not _alive("t1-reader")


def test_four_readers_yield_every_item_once_and_skip_leaks_no_slot():
    def run_pass(skip):
        made = []

        def make():
            made.append(bytearray(1))
            return made[-1]

        def read(i, slot):
            return SKIP if skip and i % 3 == 0 else i

        got = []
        with ReadAhead(50, read, make, n_readers=4, n_slots=6, name="t2-reader") as reads:
            for i, slot, payload in reads:
                assert payload == i
                got.append(i)
                reads.release(slot, Event(done=True))
        assert len(made) == 6
        return got

    assert sorted(_within(lambda: run_pass(False))) == list(range(50))
    assert sorted(_within(lambda: run_pass(True))) == [i for i in range(50) if i % 3]
    assert sorted(_within(lambda: run_pass(True))) == [i for i in range(50) if i % 3]       # a second pass completes
    assert not _alive("t2-reader")


def test_only_the_oldest_unfinished_event_is_synchronised():
    log = []

    def consume():
        events = []
        with ReadAhead(4, lambda i, slot: i, lambda: bytearray(1), n_slots=2, name="t3-reader") as reads:
            it = iter(reads)
            for k in range(2):                                        # both slots out, both released behind unfinished events
                i, slot, _ = next(it)
                events.append(Event(done=False, log=log, tag=k))
                reads.release(slot, events[-1])
            i, slot, _ = next(it)                                     # the reader has no slot: the oldest event is waited for
            assert i == 2 and log == [0] and events[1].synced == 0
            done = Event(done=True, log=log, tag="done")
            reads.release(slot, done)
            events[1].done = True                                     # finished by itself: handed back without a synchronize()
            assert next(it)[0] == 3
            assert next(it, None) is None
        assert log == [0] and done.synced == 0 and events[1].synced == 0

    _within(consume)
    assert not _alive("t3-reader")


def test_a_readers_exception_is_re_raised_by_the_iteration():
    def read(i, slot):
        if i == 3:
            raise KeyError("item 3 (injected)")
        return i

    def consume():
        got = []
        for i, slot, _ in (reads := ReadAhead(6, read, lambda: bytearray(1), n_readers=2, n_slots=3, name="t4-reader")):
            got.append(i)
            reads.release(slot, Event(done=True))
        return got

    with pytest.raises(KeyError, match="item 3"):
        _within(consume)
    assert _ended("t4-reader")


def test_a_consumer_that_stops_early_ends_the_readers():
    def consume():
        reads = ReadAhead(20, lambda i, slot: i, lambda: bytearray(1), n_readers=3, n_slots=2, name="t5-reader")
        it = iter(reads)
        first = next(it)                                              # never released: with the other slot filled, every reader waits for one
        t0 = time.monotonic()
        while reads._starved < 2 and time.monotonic() - t0 < TIMEOUT:
            time.sleep(0.005)
        assert reads._starved >= 2
        it.close()
        return first[0]

    assert _within(consume) in range(20)
    assert _ended("t5-reader")


def test_write_behind_waits_for_the_event_and_keeps_submit_order():
    order = []

    class Ev(Event):
        def synchronize(self):
            order.append(("sync", self.tag))
            time.sleep(0.01)
            super().synchronize()
            order.append(("synced", self.tag))

    def write(slot, payload):
        order.append(("write", payload, slot[0]))

    def produce():
        wb = WriteBehind(write, lambda: bytearray(1), n_writers=1, n_slots=2, name="t6-writer")
        for k in range(5):
            slot = wb.take()
            slot[0] = k
            wb.submit(slot, Ev(done=False, tag=k), k)
        wb.close()

    _within(produce)
    assert order == [e for k in range(5) for e in (("sync", k), ("synced", k), ("write", k, k))]
    assert not _alive("t6-writer")


def test_write_behind_re_raises_a_writers_exception_and_unblocks_take():
    gate = threading.Event()

    def write(slot, payload):
        if payload == 1:
            assert gate.wait(TIMEOUT)
            raise OSError("disk full (injected)")

    def produce():
        wb = WriteBehind(write, lambda: bytearray(1), n_writers=1, n_slots=2, name="t7-writer")
        try:
            for k in range(2):
                wb.submit(wb.take(), Event(), k)                      # the second write blocks on the gate: one slot stays out
            wb.submit(wb.take(), Event(), 2)                          # both slots out now
            threading.Timer(0.05, gate.set).start()
            with pytest.raises(OSError, match="injected"):
                wb.take()                                             # blocked when the writer fails: returns by raising
            with pytest.raises(OSError, match="injected"):
                wb.submit(None, Event(), 3)
            with pytest.raises(OSError, match="injected"):
                wb.take()
        finally:
            with pytest.raises(OSError, match="injected"):
                wb.close()

    _within(produce)
    assert not _alive("t7-writer")


def test_write_behind_close_joins_every_writer_and_takes_one_off_buffers():
    written = []

    def produce():
        wb = WriteBehind(lambda slot, payload: written.append((slot, payload)), lambda: bytearray(1), n_writers=3, n_slots=2, name="t8-writer")
        assert len(_alive("t8-writer")) == 3
        wb.submit(None, Event(done=False), "own buffer")              # no slot: nothing is handed back
        wb.close()
        assert wb._free.qsize() == 2

    _within(produce)
    assert written == [(None, "own buffer")] and not _alive("t8-writer")
