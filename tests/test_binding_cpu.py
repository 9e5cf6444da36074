"""binding.py on a plain Python stand-in for the library: no device, no built library."""
import ctypes as C
import gc

import numpy as np
import pytest


class _Fn:
    def __init__(self, result=0):
        self.result, self.calls = result, []

    def __call__(self, *args):
        self.calls.append(args)
        if isinstance(self.result, Exception):
            raise self.result
        return self.result


class _Lib:
    """Holds the symbols it is given; any other is an AttributeError, as on a CDLL."""

    def __init__(self, *names, **results):
        self.reads = []
        for name in names:
            self.__dict__[name] = _Fn()
        for name, result in results.items():
            self.__dict__[name] = _Fn(result)

    def __getattribute__(self, name):
        if not name.startswith("_") and name != "reads":
            object.__getattribute__(self, "reads").append(name)
        return object.__getattribute__(self, name)


PROTOS = {"x_last_error": (C.c_char_p, []), "x_make": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]), "x_destroy": (C.c_int, [C.c_void_p])}


@pytest.fixture(scope="module")
def b(pkg):
    return pkg.binding


def test_attach_sets_both_attributes_and_names_a_missing_symbol(b):
    lib = _Lib(*PROTOS)
    b.attach(lib, PROTOS)
    for name, (res, args) in PROTOS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes is args
    with pytest.raises(AttributeError, match="x_destroy"):
        b.attach(_Lib("x_last_error", "x_make"), PROTOS)


def test_binder_attaches_once_per_library_object(b):
    first, second = _Lib(*PROTOS), _Lib(*PROTOS)
    current, also = [first], []
    _lib = b.binder(PROTOS, "x", lambda: current[0], also=(lambda: also.append(1),))
    assert _lib() is first and sorted(first.reads) == sorted(PROTOS) and first._x_ready is True
    for _ in range(3):
        assert _lib() is first
    assert sorted(first.reads) == sorted(PROTOS) and also == [1], "attached once: O(1) afterwards"
    current[0] = second  # (a library loaded from an explicit path: its own flag)
    assert _lib() is second and sorted(second.reads) == sorted(PROTOS) and also == [1, 1]
    assert not hasattr(second, "_y_ready")
    other = b.binder({"x_make": PROTOS["x_make"]}, "y", lambda: second)
    assert other() is second and second._y_ready is True and second.reads.count("x_make") == 2, "one flag per tag"


def test_checker_reproduces_the_three_message_shapes(b):
    lib = _Lib(ivf_last_error=b"null index", gann_last_error=b"k must be in 1..1024", opq_last_error=b"null index")

    class IvfError(RuntimeError):
        pass

    plain = b.checker(IvfError, "ivf_ann", "ivf_last_error")
    assert plain(lib, 0) is None and lib.reads == [], "a zero status reads nothing"
    with pytest.raises(IvfError) as e:
        plain(lib, 1)
    assert str(e.value) == "ivf_ann error 1: null index"

    class GroupedError(RuntimeError):  # as grouped_ann.GroupedError, faiss_files.FaissFileError, shard_set.ShardSetError
        def __init__(self, code, message):
            super().__init__(f"grouped_ann error {code}: {message}")
            self.code, self.message = code, message

    coded = b.checker(GroupedError, "grouped_ann", "gann_last_error", with_code=True)
    with pytest.raises(GroupedError) as e:
        coded(lib, 3)
    assert str(e.value) == "grouped_ann error 3: k must be in 1..1024"
    assert (e.value.code, e.value.message) == (3, "k must be in 1..1024")

    by_prefix = b.checker(IvfError, "polysemous_ann", None)  # polysemous_ann: the last_error of the prefix in use
    assert by_prefix(lib, 0, lib.opq_last_error) is None
    with pytest.raises(IvfError) as e:
        by_prefix(lib, 2, lib.opq_last_error)
    assert str(e.value) == "polysemous_ann error 2: null index"


def test_checker_on_the_package_error_classes(pkg, b):
    lib = _Lib(e=b"why")
    for cls, label in [(pkg.faiss_files.FaissFileError, "faiss_files"), (pkg.shard_set.ShardSetError, "shard_set")]:
        with pytest.raises(cls) as e:
            b.checker(cls, label, "e", with_code=True)(lib, 1)
        assert str(e.value) == f"{label} error 1: why" and (e.value.code, e.value.message) == (1, "why")
    with pytest.raises(pkg.grouped_ann.GroupedError) as e:
        b.checker(pkg.grouped_ann.GroupedError, "grouped_ann", "e", with_code=True)(lib, 1)
    assert str(e.value) == "grouped_ann error 1: why" and e.value.code == 1


def _handle_class(b, lib):
    class Thing(b.Handle):
        _destroy, _lib = "x_destroy", staticmethod(lambda: lib)
        closed = 0

        def __init__(self, handle):
            self._h = handle

        def _closed(self):
            self.closed += 1

    return Thing


def test_handle_close_destroys_once(b):
    lib = _Lib("x_destroy")
    t = _handle_class(b, lib)(C.c_void_p(5))
    assert t._owned is True
    t.close()
    t.close()
    assert t._h is None and len(lib.x_destroy.calls) == 1 and lib.x_destroy.calls[0][0].value == 5 and t.closed == 1
    never_opened = _handle_class(b, lib)(None)
    never_opened.close()
    assert len(lib.x_destroy.calls) == 1 and never_opened.closed == 0


def test_close_forgets_the_handle_before_a_raising_destroy(b):
    lib = _Lib(x_destroy=RuntimeError("the library is gone"))
    t = _handle_class(b, lib)(5)
    with pytest.raises(RuntimeError):
        t.close()
    t.close()
    assert t._h is None and len(lib.x_destroy.calls) == 1, "at most once, whatever destroy did"


def test_a_disowned_handle_is_never_destroyed(b):
    lib = _Lib("x_destroy")
    Thing = _handle_class(b, lib)
    t = Thing(7)

    class Owner(Thing):  # as FaissRefineFlat over its base: the C side of handle 8 destroys handle 7 with itself
        def _closed(self):
            t._h = None

    owner = Owner(8)
    t._disown()
    t.close()
    assert t._h == 7 and t._owned is False and lib.x_destroy.calls == [] and t.closed == 0, "a view: usable, close() does nothing"
    owner.close()
    assert t._h is None and owner._h is None and lib.x_destroy.calls == [(8,)]
    t.close()
    owner.close()
    assert lib.x_destroy.calls == [(8,)]


def test_take_moves_handle_and_duty(b):
    lib = _Lib("x_destroy")
    Thing = _handle_class(b, lib)
    giver, taker = Thing(9), Thing(None)
    taker._take(giver)
    assert giver._h is None and giver._owned is False and taker._h == 9 and taker._owned is True
    giver.close()
    assert lib.x_destroy.calls == []
    taker.close()
    assert lib.x_destroy.calls == [(9,)]


def test_what_is_no_longer_owned_is_not_given_again(b):
    lib = _Lib("x_destroy")
    Thing = _handle_class(b, lib)
    wrapped = Thing(3)
    wrapped._disown()
    with pytest.raises(ValueError, match="given its handle away"):
        wrapped._disown()
    with pytest.raises(ValueError, match="given its handle away"):
        Thing(None)._take(wrapped)
    assert wrapped._h == 3, "the refusal changes nothing"
    giver, first, second = Thing(4), Thing(None), Thing(None)
    first._take(giver)
    with pytest.raises(ValueError, match="given its handle away"):
        second._take(giver)
    with pytest.raises(ValueError, match="given its handle away"):
        giver._disown()
    assert second._h is None and first._h == 4
    for t in (wrapped, giver, first, second):
        t.close()
    assert lib.x_destroy.calls == [(4,)]


def test_del_swallows_a_raising_destroy(b):
    lib = _Lib(x_destroy=RuntimeError("the library is gone"))
    t = _handle_class(b, lib)(11)
    t.__del__()  # no exception
    assert len(lib.x_destroy.calls) == 1
    del t
    gc.collect()
    assert len(lib.x_destroy.calls) == 1
    half_made = object.__new__(_handle_class(b, lib))  # __init__ never ran: nothing to destroy, nothing raised
    half_made.__del__()


def test_rows(b, pkg):
    assert pkg.ivf_ann._rows is b.rows and pkg.grouped_ann._rows is b.rows
    one = b.rows([1, 2, 3])
    assert one.shape == (1, 3) and one.dtype == np.float32, "a 1-D input is one row"
    x = np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]
    v = b.rows(x, 2)
    assert v.shape == (3, 2) and v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] and np.array_equal(v, x)
    f = np.zeros((2, 4), np.float32)
    assert b.rows(f, 4) is f or np.shares_memory(b.rows(f, 4), f)
    with pytest.raises(ValueError) as e:
        b.rows(np.zeros((3, 4)), 5)
    assert str(e.value) == "expected rows of dimension 5, got shape (3, 4)"
    with pytest.raises(ValueError) as e:
        b.rows(np.zeros((2, 3, 4)))
    assert str(e.value) == "expected rows of dimension None, got shape (2, 3, 4)"


def test_result_triple(b):
    ids, dist, cnt = b.result_triple(3, 4)
    assert (ids.dtype, dist.dtype, cnt.dtype) == (np.int64, np.float32, np.int32)
    assert (ids.shape, dist.shape, cnt.shape) == ((3, 4), (3, 4), (3,))
    assert not ids.any() and not dist.any() and not cnt.any()
    ids, dist, cnt = b.result_triple(2, -1, clamp=True)  # shard_set, annoy_ann: the library refuses k, not numpy
    assert (ids.shape, dist.shape, cnt.shape) == ((2, 0), (2, 0), (2,))
    with pytest.raises(ValueError):
        b.result_triple(2, -1)


def test_ids_or_none_and_ptr(b):
    assert b.ids_or_none(None, 5) is None and b.ptr(None) is None
    ids = b.ids_or_none(range(4), 4)
    assert ids.dtype == np.int64 and ids.shape == (4,) and ids.tolist() == [0, 1, 2, 3] and b.ptr(ids) == ids.ctypes.data
    for bad in (range(3), np.zeros((4, 1))):
        with pytest.raises(ValueError) as e:
            b.ids_or_none(bad, 4)
        assert str(e.value) == "one id per vector"
    with pytest.raises(ValueError) as e:
        b.ids_or_none([1], 2, "row")
    assert str(e.value) == "one id per row"
