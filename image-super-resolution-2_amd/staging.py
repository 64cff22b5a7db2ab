"""Host staging between disk, pinned memory and the device: the only module that starts a staging thread.  Worker threads fill
(ReadAhead) or drain (WriteBehind) slots and make no GPU call; the calling thread owns every GPU call and says, with an event recorded
behind its last copy, when a slot may be used again.  An event is any object with query() and synchronize() (torch.cuda.Event); a
slot is whatever make_slot() returns, made on the constructing thread because pinning is a GPU call.  Nothing here imports torch."""
from __future__ import annotations

import queue
import threading
import time

SKIP = object()                                                       # read() -> SKIP: nothing to hand on, the slot goes straight back


class ReadAhead:
    """n_readers threads take the items 0 .. n_items-1 in turn from one counter, each with a free slot, and call read(i, slot) -> payload.
    Iterating yields (i, slot, payload) on the calling thread -- item order with one reader, arrival order with several -- and
    release(slot, event) gives a slot back.  Slots are recycled on the calling thread: those whose event reports query() when the next
    item is asked for, and the oldest is synchronize()d only when nothing is ready while a reader waits for a slot and none is free.
    A reader's exception ends the iteration and is re-raised by it.  close() -- the end of the iteration, generator close() or context
    exit -- stops and joins the readers and waits for the events still pending.
    wait_s: seconds the calling thread blocked for an item; busy_s: the readers' seconds inside read()."""

    def __init__(self, n_items, read, make_slot, n_readers=1, n_slots=None, name="ff-reader"):
        self._n, self._read, self._cv = int(n_items), read, threading.Condition()
        self._free = [make_slot() for _ in range(n_readers + 2 if n_slots is None else n_slots)]
        self._ready, self._pending = [], []                           # (i, slot, payload) read; (event, slot) released, not known done
        self._next = self._starved = 0                                # next item number; readers waiting for a slot
        self._err, self._stop, self._live = None, False, n_readers
        self.wait_s = self.busy_s = 0.0
        self._threads = [threading.Thread(target=self._run, name=f"{name}{k}", daemon=True) for k in range(n_readers)]
        for t in self._threads:
            t.start()

    def _run(self):
        starving = lambda: not self._free and not self._stop and self._next < self._n      # noqa: E731 -- asked under the lock
        try:
            while True:
                with self._cv:
                    if starving():
                        self._starved += 1                            # told to the calling thread once, not per wake-up
                        self._cv.notify_all()
                        while starving():
                            self._cv.wait()
                        self._starved -= 1
                    if self._stop or self._next >= self._n:
                        return
                    i, slot = self._next, self._free.pop()
                    self._next += 1
                t0 = time.perf_counter()
                payload = self._read(i, slot)
                with self._cv:
                    self.busy_s += time.perf_counter() - t0
                    if payload is SKIP:
                        self._free.append(slot)
                    else:
                        self._ready.append((i, slot, payload))
                    self._cv.notify_all()
        except BaseException as e:                                    # noqa: BLE001 -- re-raised on the calling thread
            self._err = e
        finally:
            with self._cv:
                self._live -= 1
                self._cv.notify_all()

    def release(self, slot, event):
        self._pending.append((event, slot))

    def _take(self):
        """The next (i, slot, payload), or None once every reader has ended."""
        with self._cv:
            for p in [p for p in self._pending if p[0].query()]:
                self._pending.remove(p)
                self._free.append(p[1])
            self._cv.notify_all()
            while True:
                if self._err is not None:
                    raise self._err
                if self._ready:
                    return self._ready.pop(0)
                if not self._live:
                    return None
                if self._starved and not self._free:
                    if not self._pending and self._starved == self._live:
                        raise RuntimeError("ReadAhead: every slot is held by the caller; release() a slot before asking for the next item")
                    if self._pending:
                        event, slot = self._pending.pop(0)
                        event.synchronize()
                        self._free.append(slot)
                        self._cv.notify_all()
                self._cv.wait()

    def __iter__(self):
        try:
            while True:
                t0 = time.perf_counter()
                item = self._take()
                self.wait_s += time.perf_counter() - t0
                if item is None:
                    return
                yield item
        finally:
            self.close()

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        for t in self._threads:
            t.join()
        for event, _ in self._pending:
            if not event.query():
                event.synchronize()
        self._pending = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class WriteBehind:
    """n_writers threads drain result slots: slot = take(); ...queue the copies into it, record `event`...; submit(slot, event, payload).
    A writer waits for the event, calls write(slot, payload) and frees the slot; a payload that carries a buffer of its own is
    submitted with slot None.  A writer's exception is re-raised by the next take(), submit() or close(); from then on the writers
    only hand slots back, so a take() that was blocked returns.  close() drains, joins and re-raises.
    wait_s: seconds take() blocked; busy_s: the writers' seconds inside write(), summed."""

    def __init__(self, write, make_slot, n_writers, n_slots, name="ff-writer"):
        self._write, self._free, self._jobs, self._lock, self._err = write, queue.Queue(), queue.Queue(), threading.Lock(), None
        for _ in range(n_slots):
            self._free.put(make_slot())
        self.wait_s = self.busy_s = 0.0
        self._threads = [threading.Thread(target=self._run, name=f"{name}{k}", daemon=True) for k in range(n_writers)]
        for t in self._threads:
            t.start()

    def _run(self):
        for slot, event, payload in iter(self._jobs.get, None):
            try:
                if self._err is None:
                    event.synchronize()
                    t0 = time.perf_counter()
                    self._write(slot, payload)
                    with self._lock:
                        self.busy_s += time.perf_counter() - t0
            except BaseException as e:                                # noqa: BLE001 -- re-raised on the calling thread
                self._err = e
            if slot is not None:
                self._free.put(slot)

    def _check(self):
        if self._err is not None:
            raise self._err

    def take(self):
        self._check()
        t0 = time.perf_counter()
        slot = self._free.get()
        self.wait_s += time.perf_counter() - t0
        self._check()
        return slot

    def submit(self, slot, event, payload=None):
        self._check()
        self._jobs.put((slot, event, payload))

    def close(self):
        for _ in self._threads:
            self._jobs.put(None)
        for t in self._threads:
            t.join()
        self._threads = []
        self._check()
