"""Host tests of the two tables behind the in-place pinning of caller arrays (femo_amd/engine.py: ``_SEEN``, ``_REGISTERED``,
``_STALE``, ``_note_caller_array``, ``register``, ``_forget_owner``, ``pin_stats``).  No GPU and no library: ``_lib.load`` is
replaced by a fake that records ``femo_host_register(addr, n)`` / ``femo_host_unregister(addr)``, keeps the set of pinned
ranges, refuses every range that intersects one (as hostmem.cpp does) and can be told to refuse the next call of either
kind.  The question throughout: can a range stay pinned after its array is gone, or an array be pinned twice, without
anybody noticing?"""
import ctypes
import gc
import threading

import numpy as np
import pytest

from femo_amd import engine

MIN_BYTES = 256
N = 64                       # doubles: 512 bytes, above the lowered threshold


class FakeLib:
    def __init__(self):
        self.pinned = {}     # address -> bytes
        self.calls = []
        self.refuse_register = False
        self.refuse_unregister = False

    def _overlaps(self, addr, n):
        return any(addr < a + b and a < addr + n for a, b in self.pinned.items())

    def femo_host_register(self, p, n):
        addr = p.value
        self.calls.append(("register", addr, n))
        if self.refuse_register:
            self.refuse_register = False
            return 1
        if n <= 0 or self._overlaps(addr, n):
            return 1
        self.pinned[addr] = n
        return 0

    def femo_host_unregister(self, p):
        addr = p.value
        self.calls.append(("unregister", addr))
        if self.refuse_unregister:
            self.refuse_unregister = False
            return 1                                         # the range stays pinned
        if addr not in self.pinned:
            return 1
        del self.pinned[addr]
        return 0

    def ranges(self):
        return set(self.pinned.items())

    def count(self, kind, addr=None):
        return sum(1 for c in self.calls if c[0] == kind and (addr is None or c[1] == addr))


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(engine._lib, "load", lambda: lib)
    monkeypatch.setattr(engine, "AUTO_REGISTER_MIN_BYTES", MIN_BYTES)
    monkeypatch.setattr(engine, "_SEEN", {})
    monkeypatch.setattr(engine, "_REGISTERED", {})
    monkeypatch.setattr(engine, "_STALE", [])
    monkeypatch.setattr(engine, "_PIN_COUNTS", dict(register_refused=0, unregister_failed=0))
    monkeypatch.setattr(engine, "_AUTO_REGISTER", True)
    yield lib
    gc.collect()


def _rng(a):
    return (a.ctypes.data, a.nbytes)


def _stats(**kw):
    want = dict(seen=0, registered=0, register_refused=0, unregister_failed=0, stale=0)
    want.update(kw)
    return want


# ------------------------------------------------------------------------------------------------ fixed scenarios ----
def test_second_sight_pins_third_does_nothing(fake):
    a = np.zeros(N)
    engine._note_caller_array(a)
    assert fake.calls == [] and engine.pin_stats() == _stats(seen=1)
    engine._note_caller_array(a)
    assert fake.calls == [("register",) + _rng(a)] and fake.ranges() == {_rng(a)}
    assert engine.pin_stats() == _stats(seen=1, registered=1)
    engine._note_caller_array(a)
    assert len(fake.calls) == 1


def test_views_count_as_their_owner(fake):
    a = np.zeros(4 * N)
    engine._note_caller_array(a[3:])
    engine._note_caller_array(a.reshape(4, N)[1:].ravel())   # a view of a view, elsewhere in the owner
    assert fake.ranges() == {_rng(a)}                        # the owner's whole range, once
    engine._note_caller_array(a[::2][5:])
    engine._note_caller_array(a)
    assert len(fake.calls) == 1
    v = a[7:]
    del a
    gc.collect()
    assert fake.count("unregister") == 0                     # the view keeps the owner alive: still pinned
    addr = next(iter(fake.pinned))
    del v
    gc.collect()
    assert fake.calls[-1] == ("unregister", addr) and fake.ranges() == set()


class _BlockLike:
    """Memory that is not NumPy's (what engine._PinnedBlock looks like to ``np.asarray``)."""

    def __init__(self, n):
        self.buf = (ctypes.c_double * n)()
        self.__array_interface__ = dict(shape=(n,), typestr="<f8", data=(ctypes.addressof(self.buf), False), version=3)


def test_foreign_memory_is_never_pinned(fake, tmp_path):
    arrays = [np.frombuffer(bytearray(8 * N), dtype=np.float64),
              np.asarray(_BlockLike(N)),
              np.asarray(_BlockLike(2 * N))[N:],
              np.memmap(str(tmp_path / "m.bin"), dtype=np.float64, mode="w+", shape=(N,))]
    for a in arrays:
        for _ in range(3):
            engine._note_caller_array(a)
        assert engine.register(a) is False
    assert fake.calls == [] and engine.pin_stats() == _stats()


def test_small_arrays_are_never_pinned(fake):
    a = np.zeros(MIN_BYTES // 8 - 1)
    for _ in range(3):
        engine._note_caller_array(a)
    assert fake.calls == [] and engine.pin_stats() == _stats()
    b = np.zeros(MIN_BYTES // 8)                             # exactly the threshold is pinned
    engine._note_caller_array(b)
    engine._note_caller_array(b)
    assert fake.ranges() == {_rng(b)}


class _MovingOwner:
    """An owner whose memory moves, as a resize in place would move it.  ``ndarray.resize`` itself cannot be the mover:
    NumPy refuses to resize an array that carries a weak reference, and every array seen once carries the finalizer's
    (test_numpy_refuses_to_resize_a_seen_array).  The tables look at ``base``, ``flags.owndata``, ``ctypes.data`` and
    ``nbytes`` only, so this object walks the path that a mover would."""

    base = None

    def __init__(self, n):
        self._old = []
        self._buf = np.zeros(n)

    flags = property(lambda self: self._buf.flags)
    ctypes = property(lambda self: self._buf.ctypes)
    nbytes = property(lambda self: self._buf.nbytes)

    def move(self, n):
        self._old.append(self._buf)                          # kept: the new memory is elsewhere for certain
        self._buf = np.zeros(n)


def test_numpy_refuses_to_resize_a_seen_array(fake):
    a = np.zeros(N)
    a.resize(2 * N, refcheck=False)                          # never handed over: free to move
    engine._note_caller_array(a)                             # first sight attaches the finalizer ...
    with pytest.raises(ValueError):
        a.resize(4096 * N, refcheck=False)                   # ... and with it NumPy's refusal
    engine._note_caller_array(a)
    with pytest.raises(ValueError):
        a.resize(4096 * N, refcheck=False)
    assert fake.ranges() == {_rng(a)} and a.size == 2 * N    # pinned where it still lives


def test_death_unpins_by_the_recorded_address_exactly_once(fake):
    a = _MovingOwner(N)
    engine._note_caller_array(a)
    engine._note_caller_array(a)
    a.move(3 * N)                                            # the move path attaches a second finalizer
    engine._note_caller_array(a)
    engine._note_caller_array(a)
    rng = _rng(a)
    assert fake.ranges() == {rng}
    del a
    gc.collect()
    assert fake.ranges() == set() and engine.pin_stats() == _stats()
    # both finalizers ran, and one call followed the death: the second finalizer found no record
    assert fake.calls[fake.calls.index(("register",) + rng) + 1:] == [("unregister", rng[0])]


def test_a_move_unpins_the_old_range_first(fake):
    a = _MovingOwner(N)
    engine._note_caller_array(a)
    engine._note_caller_array(a)
    old = _rng(a)
    a.move(3 * N)
    new = _rng(a)
    assert new[0] != old[0]
    engine._note_caller_array(a)                             # a first sight again, but the old pin goes now
    assert fake.calls[-1] == ("unregister", old[0]) and fake.ranges() == set()
    assert engine.pin_stats() == _stats(seen=1)
    engine._note_caller_array(a)
    assert fake.calls[-1] == ("register",) + new and fake.ranges() == {new}
    b = _MovingOwner(N)
    assert engine.register(b)
    b_old = _rng(b)
    b.move(N)                                                # the same size elsewhere
    assert engine.register(b)                                # register() goes the same way
    assert fake.calls[-2:] == [("unregister", b_old[0]), ("register",) + _rng(b)]
    assert fake.ranges() == {new, _rng(b)}


def test_a_reused_id_starts_from_first_sight(fake):
    a = np.zeros(N)
    engine._note_caller_array(a)
    engine._note_caller_array(a)
    key = id(a)
    del a
    gc.collect()
    assert key not in engine._SEEN and key not in engine._REGISTERED and fake.ranges() == set()
    keep = []
    for _ in range(64):                                      # CPython hands a freed object's slot out again soon
        b = np.zeros(N)
        if id(b) == key:
            break
        keep.append(b)
    ncalls = len(fake.calls)
    engine._note_caller_array(b)
    assert len(fake.calls) == ncalls                         # first sight, whatever its id
    engine._note_caller_array(b)
    assert fake.calls[-1] == ("register",) + _rng(b)


def test_a_refused_register_is_tried_again(fake):
    a = np.zeros(N)
    engine._note_caller_array(a)
    fake.refuse_register = True
    engine._note_caller_array(a)
    assert fake.count("register") == 1 and fake.ranges() == set()
    assert id(a) not in engine._SEEN and id(a) not in engine._REGISTERED
    assert engine.pin_stats() == _stats(register_refused=1)
    engine._note_caller_array(a)
    assert fake.count("register") == 1
    engine._note_caller_array(a)
    assert fake.count("register") == 2 and fake.ranges() == {_rng(a)}
    b = np.zeros(N)
    fake.refuse_register = True
    assert engine.register(b) is False
    assert id(b) not in engine._SEEN and id(b) not in engine._REGISTERED
    assert engine.pin_stats() == _stats(seen=1, registered=1, register_refused=2)
    rng = _rng(a)
    del a
    gc.collect()
    assert fake.calls[-1] == ("unregister", rng[0])          # the finalizer of the first attempt still serves


def test_a_refused_unregister_is_kept_and_blocks_the_range(fake):
    a = np.zeros(N)
    assert engine.register(a)
    rng = _rng(a)
    fake.refuse_unregister = True
    del a
    gc.collect()
    assert fake.calls[-1] == ("unregister", rng[0]) and fake.ranges() == {rng}        # the pin outlived its array
    assert engine._STALE == [rng]
    assert engine.pin_stats() == _stats(unregister_failed=1, stale=1)
    # an owner on that range (here: an array laid over it on purpose) is never pinned again
    ncalls = len(fake.calls)

    hold = np.zeros(4 * N)
    engine._STALE[0] = (hold.ctypes.data + 8, 16)            # move the stale range into memory this test owns
    for _ in range(3):
        engine._note_caller_array(hold)
    assert engine.register(hold) is False
    assert len(fake.calls) == ncalls and id(hold) not in engine._SEEN and id(hold) not in engine._REGISTERED
    other = np.zeros(N)                                      # elsewhere: pinned as usual
    engine._note_caller_array(other)
    engine._note_caller_array(other)
    assert fake.calls[-1] == ("register",) + _rng(other)


def test_auto_register_off_pins_and_unpins_nothing(fake):
    a = np.zeros(N)
    engine._note_caller_array(a)
    engine._note_caller_array(a)
    engine.auto_register(False)
    try:
        assert fake.ranges() == {_rng(a)}                    # switching off unpins nothing
        b = np.zeros(N)
        for _ in range(3):
            engine._note_caller_array(b)
        assert len(fake.calls) == 1 and id(b) not in engine._SEEN
    finally:
        engine.auto_register(True)
    engine._note_caller_array(b)
    assert len(fake.calls) == 1                              # nothing was counted meanwhile: a first sight


def test_register_on_a_pinned_owner_is_one_call(fake):
    a = np.zeros(N)
    assert engine.register(a) is True
    assert engine.register(a) is True and engine.register(a[5:]) is True
    engine._note_caller_array(a)
    assert fake.calls == [("register",) + _rng(a)]
    small = np.zeros(2)
    assert engine.register(small) is True                    # an explicit request has no size threshold
    assert engine.pin_stats() == _stats(seen=2, registered=2)


# ---------------------------------------------------------------------------------------------------- random walk ----
class Model:
    """What the tables must hold, restated per pool slot: ``seen`` and ``reg`` are (address, bytes) or None."""

    def __init__(self, slots):
        self.seen = [None] * slots
        self.reg = [None] * slots
        self.ever = [False] * slots                          # the slot's array was seen at least once: it has a finalizer

    # the registry as the fake must see it, from all models of a test
    @staticmethod
    def pinned(models, stale):
        out = set(stale)
        for m in models:
            out |= {r for r in m.reg if r is not None}
        return out

    def forget(self, i, shared, dead=True):
        rec, self.seen[i], self.reg[i] = self.reg[i], None, None
        if dead:
            self.ever[i] = False
        if rec is not None and shared["refuse_unregister"]:
            shared["refuse_unregister"] = False
            shared["stale"].append(rec)
            shared["unregister_failed"] += 1

    def _try(self, i, rng, shared, models):
        hit = any(rng[0] < a + b and a < rng[0] + rng[1] for a, b in Model.pinned(models, shared["stale"]))
        if shared["refuse_register"] or hit:
            shared["refuse_register"] = False
            shared["register_refused"] += 1
            self.seen[i] = None
            return False
        self.reg[i] = rng
        return True

    @staticmethod
    def _stale_hit(rng, shared):
        return any(rng[0] < a + b and a < rng[0] + rng[1] for a, b in shared["stale"])

    def note(self, i, rng, shared, models):
        if not shared["auto"] or rng[1] < MIN_BYTES:
            return
        if self.reg[i] is not None:
            if self.reg[i] == rng:
                return
            self.forget(i, shared, dead=False)
        if self._stale_hit(rng, shared):
            self.seen[i] = None
            return
        self.ever[i] = True
        if self.seen[i] != rng:
            self.seen[i] = rng
            return
        self._try(i, rng, shared, models)

    def register(self, i, rng, shared, models):
        if self.reg[i] == rng:
            return True
        if self.reg[i] is not None:
            self.forget(i, shared, dead=False)
        if self._stale_hit(rng, shared):
            self.seen[i] = None
            return False
        self.ever[i] = True
        self.seen[i] = rng
        return self._try(i, rng, shared, models)


def _shared():
    return dict(auto=True, refuse_register=False, refuse_unregister=False, stale=[], register_refused=0, unregister_failed=0)


def _view(rs, a):
    k = rs.integers(4)
    if k == 0 or a.size < 8:
        return a
    if k == 1:
        return a[int(rs.integers(1, a.size // 2)):]
    if k == 2:
        return a.reshape(2, -1)[1]
    return a[1:][2:]


def _walk(fake, rs, model, models, shared, steps, full, check):
    pool = [None] * len(model.seen)
    sizes = (N, N, 2 * N, 3 * N, MIN_BYTES // 8 - 2)
    for _ in range(steps):
        i = int(rs.integers(len(pool)))
        op = int(rs.integers(10 if full else 6))
        a = pool[i]
        if a is None:
            pool[i] = np.zeros(sizes[int(rs.integers(len(sizes)))])
        elif op <= 2:
            engine._note_caller_array(_view(rs, a))
            model.note(i, _rng(a), shared, models)
        elif op == 3:
            assert engine.register(_view(rs, a)) == model.register(i, _rng(a), shared, models)
        elif op <= 5:
            a = pool[i] = None                               # the last reference: the finalizers run here
            model.forget(i, shared)
        elif op == 6:
            before = _rng(a)
            try:
                a.resize(int(rs.integers(1, 6)) * N, refcheck=False)
            except ValueError:                               # NumPy's refusal: only for arrays that carry a finalizer
                assert model.ever[i] and _rng(a) == before
            else:
                assert not model.ever[i] or _rng(a) == before
            engine._note_caller_array(a)
            model.note(i, _rng(a), shared, models)
        elif op == 7:
            fake.refuse_register = shared["refuse_register"] = True
        elif op == 8 and len(shared["stale"]) < 3:
            fake.refuse_unregister = shared["refuse_unregister"] = True
        elif op == 9:
            shared["auto"] = False                           # off for a few sights (no resize meanwhile: it could not be shown)
            engine.auto_register(False)
            for j in rs.integers(len(pool), size=3):
                if pool[j] is not None:
                    engine._note_caller_array(pool[j])
                    model.note(int(j), _rng(pool[j]), shared, models)
            shared["auto"] = True
            engine.auto_register(True)
        del a
        check(pool)
    return pool


def _disjoint(ranges):
    r = sorted(ranges)
    return all(r[k][0] + r[k][1] <= r[k + 1][0] for k in range(len(r) - 1))


def test_random_walk_keeps_tables_and_registry_in_step(fake):
    rs = np.random.default_rng(2024)
    shared = _shared()
    model = Model(8)

    def check(pool):
        want = Model.pinned([model], shared["stale"])
        assert fake.ranges() == want
        assert _disjoint(want)
        assert engine.pin_stats() == dict(seen=sum(s is not None for s in model.seen),
                                          registered=sum(r is not None for r in model.reg),
                                          register_refused=shared["register_refused"],
                                          unregister_failed=shared["unregister_failed"], stale=len(shared["stale"]))
        for i, a in enumerate(pool):                         # a pinned slot is pinned where its array lives now
            if model.reg[i] is not None:
                assert a is not None and model.reg[i] == _rng(a)

    pool = _walk(fake, rs, model, [model], shared, 2000, True, check)
    assert fake.count("register") > 100 and fake.count("unregister") > 50 and shared["register_refused"] > 0
    assert shared["unregister_failed"] > 0
    for i in range(len(pool)):
        pool[i] = None
        model.forget(i, shared)
    check(pool)
    assert fake.ranges() == set(shared["stale"])             # nothing outlives its array but what the fake refused to let go


def test_random_walk_from_four_threads(fake):
    shared = _shared()
    models = [Model(8) for _ in range(4)]
    errors = []

    def run(t):
        rs = np.random.default_rng(100 + t)
        m = models[t]

        def check(pool):                                     # this thread's slots only: the others move meanwhile
            for i, a in enumerate(pool):
                if m.reg[i] is not None:
                    assert fake.pinned.get(m.reg[i][0]) == m.reg[i][1] and m.reg[i] == _rng(a)
                elif a is not None:
                    assert a.ctypes.data not in fake.pinned

        try:
            pool = _walk(fake, rs, m, models, shared, 500, False, check)
            for i in range(len(pool)):
                pool[i] = None
                m.forget(i, shared)
        except BaseException as e:                           # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:
        raise errors[0]
    assert fake.count("register") > 100
    assert fake.ranges() == set() and engine.pin_stats() == _stats()
    regs = [c for c in fake.calls if c[0] == "register"]
    assert len(regs) == fake.count("unregister")             # every pin was taken back, once
