"""The footprint checker (tests/guarded.py) is itself tested first, on the CPU: the numpy backend and small fake
"filters" written in numpy. A well-behaved fake passes; every misbehaving one fails with the right plane and offset in
the message. The fakes are ordinary host code working on host memory."""
import ctypes as C
import re

import numpy as np
import pytest

import guarded as G


def _view(arena, name, rows=None, cols=None, back=0):
    """what a kernel sees: the plane's memory from (base - back samples) on, as a (rows, pitch) array over the arena's host memory"""
    s = arena.spec(name)
    rows = s.h if rows is None else rows
    n = rows * s.pitch + back
    buf = (C.c_char * (n * s.isz)).from_address(arena.address(name) - back * s.isz)
    flat = np.frombuffer(buf, s.dtype)
    return flat if back else flat.reshape(rows, s.pitch)


def _src(h, w, dtype, seed=3):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 200, (h, w)).astype(dtype)


def _specs(h=12, w=21, dtype=np.uint8, pitch=32, shift=0, in_place=False):
    def make():
        a = _src(h, w, dtype)
        if in_place:
            return [G.PlaneSpec("p", "inout", h, w, dtype, pitch, shift, data=a)]
        return [G.PlaneSpec("src", "in", h, w, dtype, pitch, shift, data=a), G.PlaneSpec("dst", "out", h, w, dtype, pitch, shift)]
    return make


def _good(arena):
    """dst = src + 1 inside [0, w) x h and nothing else"""
    s = arena.spec("src")
    _view(arena, "dst")[:, :s.w] = _view(arena, "src")[:, :s.w] + 1


def _expect(specs):
    return {"dst": next(s for s in specs if s.name == "src").data + 1}


def _run(call, make=None, **kw):
    return G.run_case(G.NumpyBackend, make or _specs(), call, _expect, **kw)


@pytest.mark.parametrize("layout", [dict(), dict(pitch=21), dict(shift=1), dict(dtype=np.uint16, pitch=24, shift=2), dict(dtype=np.float32, pitch=21)])
def test_well_behaved_filter_passes(layout):
    outs, _ = _run(_good, _specs(**layout))
    assert np.array_equal(outs["dst"], _src(12, 21, layout.get("dtype", np.uint8)) + 1)


def _fails(call, pattern, make=None, **kw):
    with pytest.raises(G.FootprintError) as e:
        _run(call, make, **kw)
    assert re.search(pattern, str(e.value)), str(e.value)
    return str(e.value)


def test_one_sample_past_w_in_the_last_row():
    def bad(arena):
        _good(arena)
        _view(arena, "dst")[11, 21] = 7
    _fails(bad, r"plane 'dst'.*write outside \[0, w\) x h: first at row 11, column 21 \(outside w = 21, pitch 32\); 1 bytes differ")


def test_one_sample_past_w_in_the_last_row_tight_pitch():
    """pitch == w: the sample after the last one is the first byte of the guard"""
    def bad(arena):
        _good(arena)
        _view(arena, "dst", rows=13)[12, 0] = 7
    _fails(bad, r"plane 'dst'.*first at 1 bytes past the end \(h x stride = 252 bytes\); 1 bytes differ", _specs(pitch=21))


def test_write_into_the_guard_before_the_plane():
    def bad(arena):
        _good(arena)
        _view(arena, "dst", back=3)[0] = 7
    _fails(bad, r"plane 'dst'.*first at 3 bytes before the plane; 1 bytes differ")


def test_write_at_h_times_stride_and_beyond():
    def bad(arena):
        _good(arena)
        v = _view(arena, "dst", rows=14)
        v[12, 0] = 7
        v[13, 5] = 7
    _fails(bad, r"plane 'dst'.*first at 1 bytes past the end \(h x stride = 384 bytes\); 2 bytes differ")


def test_u16_offsets_are_in_samples_and_bytes():
    def bad(arena):
        _good(arena)
        _view(arena, "dst")[4, 22] = 0x0101
    _fails(bad, r"plane 'dst' \(out, 12x21 uint16.*first at row 4, column 22 .*; 2 bytes differ", _specs(dtype=np.uint16))


def test_input_plane_modified():
    def bad(arena):
        _good(arena)
        _view(arena, "src")[5, 9] ^= 0xFF
    _fails(bad, r"plane 'src' \(in,.*input plane modified: first at row 5, column 9; 1 bytes differ")


def test_input_padding_written():
    def bad(arena):
        _good(arena)
        _view(arena, "src")[5, 30] = 9
    _fails(bad, r"plane 'src' \(in,.*write outside \[0, w\) x h: first at row 5, column 30")


def test_wrong_value_is_named_with_row_and_column():
    def bad(arena):
        _good(arena)
        _view(arena, "dst")[3, 4] += 1
    _fails(bad, r"plane 'dst'.*output differs from the oracle: first at row 3, column 4; 1 bytes differ")


def _rowsum_specs():
    a = _src(12, 21, np.uint16)
    return [G.PlaneSpec("src", "in", 12, 21, np.uint16, 32, data=a), G.PlaneSpec("dst", "out", 12, 21, np.uint16, 32)]


def test_padded_column_in_a_row_sum_passes_zeros_and_fails_the_poison_comparison():
    """a window sum that takes one padded column: right under poison 0x00, caught by the 0x00 / 0xFF comparison"""
    def filt(take):
        def f(arena):
            src = _view(arena, "src").astype(np.uint32)
            _view(arena, "dst")[:, :21] = (src[:, :21] + src[:, take:take + 1].sum(axis=1, keepdims=True)).astype(np.uint16)
        return f

    def expect(specs):
        a = specs[0].data.astype(np.uint32)
        return {"dst": (a + a[:, 20:21]).astype(np.uint16)}

    G.run_case(G.NumpyBackend, _rowsum_specs, filt(20), expect)  # sums the last real column
    # the 0x00 run alone is fine with column 21 (zeros) added on top: check that, then the whole protocol
    arena = G.Arena(G.NumpyBackend(), _rowsum_specs(), 0x00)

    def both(arena):
        src = _view(arena, "src").astype(np.uint32)
        _view(arena, "dst")[:, :21] = (src[:, :21] + src[:, 20:22].sum(axis=1, keepdims=True)).astype(np.uint16)
    both(arena)
    arena.check(arena.backend.copy_out(), expect(arena.specs))
    with pytest.raises(G.FootprintError) as e:
        G.run_case(G.NumpyBackend, _rowsum_specs, both, expect)
    assert re.search(r"plane 'dst'.*output differs from the oracle: first at row 0, column 0.*poison 0xFF", str(e.value)), str(e.value)


def test_padding_that_changes_nothing_under_the_oracle_still_fails_the_comparison_of_the_two_runs():
    """an output that is 'right' under either poison by the file's rule but differs between them is a dependence"""
    def filt(arena):
        _good(arena)
        pad = int(_view(arena, "src")[0, 25])
        _view(arena, "dst")[2, 2] += pad & 1  # 0 under 0x00, 1 under 0xFF

    def same(name, got, want):  # a rule with a tolerance of one unit
        return np.abs(got.astype(int) - want.astype(int)).max() <= 1
    with pytest.raises(G.FootprintError) as e:
        _run(filt, same=same)
    assert re.search(r"plane 'dst': output depends on bytes outside \[0, w\) x h.*first at row 2, column 2; 1 bytes differ", str(e.value)), str(e.value)


def test_scalars_must_not_depend_on_the_poison():
    def reader(arena):
        return [float(_view(arena, "src")[:, :22].astype(np.float64).sum())]  # one padded column too many
    make = lambda: _specs()()[:1]
    with pytest.raises(G.FootprintError) as e:
        G.run_case(G.NumpyBackend, make, reader, {})
    assert "scalars depend on bytes outside" in str(e.value)
    _, v = G.run_case(G.NumpyBackend, make, lambda a: [float(_view(a, "src")[:, :21].astype(np.float64).sum())], {})
    assert v == [float(_src(12, 21, np.uint8).astype(np.float64).sum())]


@pytest.mark.parametrize("shift,pitch,aligned", [(0, 32, True), (1, 32, False), (0, 27, False), (16, 48, True)])
def test_tail_group_write_passes_iff_granted_and_16_byte_aligned(shift, pitch, aligned):
    """the one exception clause 3 could grant: up to the end of the 16-byte group holding column w - 1, inside the pitch"""
    def tail(arena):
        _good(arena)
        _view(arena, "dst")[:, 21:min(32, pitch)] = 5
    make = _specs(shift=shift, pitch=pitch)
    if aligned:
        _run(tail, make, grant_tail=True)
    else:
        _fails(tail, r"plane 'dst'.*write outside \[0, w\) x h: first at row 0, column 21", make, grant_tail=True)
    _fails(tail, r"plane 'dst'.*first at row 0, column 21", make, grant_tail=False)  # and never while the clause is strict
    assert G.TAIL_GROUP_GRANTED is False  # the header's clause 3 is strict; see guarded.py


def test_tail_group_grant_ends_at_the_group():
    def wide(arena):
        _good(arena)
        _view(arena, "dst")[:, 21:33] = 5
    _fails(wide, r"plane 'dst'.*first at row 0, column 32", _specs(pitch=48), grant_tail=True)


def _window_specs(role_in_window=True):
    def make():
        rng = np.random.default_rng(5)
        H, W, y0, x0, h, w = 20, 40, 3, 7, 12, 21
        nb = rng.integers(1, 250, (H, W)).astype(np.uint8)
        a = nb[y0:y0 + h, x0:x0 + w].copy()
        return [G.PlaneSpec("src", "in", h, w, np.uint8, 48, 0, data=a, window=(H, W, y0, x0), neighbours=nb),
                G.PlaneSpec("dst", "out", h, w, np.uint8, 48, 0, window=(H, W, y0, x0), neighbours=nb[::-1].copy())]
    return make


def test_window_neighbours_must_survive():
    _run(_good, _window_specs())

    def bad(arena):
        _good(arena)
        _view(arena, "dst")[6, 21] = 0  # the live sample right of the window
    _fails(bad, r"plane 'dst'.*write outside \[0, w\) x h: first at row 6, column 21", _window_specs())

    def above(arena):
        _good(arena)
        _view(arena, "dst", back=48)[0] = 0  # the live sample above (0, 0)
    _fails(above, r"plane 'dst'.*first at 48 bytes before the plane", _window_specs())


def test_packed_planes_name_the_right_plane():
    def make():
        out = []
        for i, (h, w) in enumerate([(5, 9), (7, 30), (3, 17), (9, 11), (4, 4)]):
            out.append(G.PlaneSpec(f"src{i}", "in", h, w, np.uint8, w, data=_src(h, w, np.uint8, i)))
            out.append(G.PlaneSpec(f"dst{i}", "out", h, w, np.uint8, w))
        return [out[k] for k in (3, 0, 9, 6, 1, 4, 7, 2, 5, 8)]

    def call(bad):
        def f(arena):
            for i in range(5):
                s = arena.spec(f"src{i}")
                _view(arena, f"dst{i}")[:, :s.w] = _view(arena, f"src{i}")[:, :s.w] + 1
            if bad:
                _view(arena, "dst2", rows=4)[3, 0] = 1
        return f
    expect = lambda specs: {s.name.replace("src", "dst"): s.data + 1 for s in specs if s.role == "in"}
    G.run_case(G.NumpyBackend, make, call(False), expect)
    with pytest.raises(G.FootprintError) as e:
        G.run_case(G.NumpyBackend, make, call(True), expect)
    assert re.search(r"plane 'dst2'.*first at 1 bytes past the end", str(e.value)), str(e.value)


def test_in_place_plane():
    """dst == src: one "inout" plane, uploaded and expected to come back as the oracle's output"""
    def call(arena):
        _view(arena, "p")[:, :21] += 1
    expect = lambda specs: {"p": specs[0].data + 1}
    G.run_case(G.NumpyBackend, _specs(in_place=True), call, expect)

    def bad(arena):
        call(arena)
        _view(arena, "p")[0, 21] = 1
    with pytest.raises(G.FootprintError) as e:
        G.run_case(G.NumpyBackend, _specs(in_place=True), bad, expect)
    assert re.search(r"plane 'p' \(inout,.*first at row 0, column 21", str(e.value)), str(e.value)


def test_rows_that_are_not_inputs_hold_poison():
    seen = []

    def make2():  # the EEDI3 shape: poisoned rows in an input, a separate output that never reads them
        a = _src(12, 21, np.uint8)
        return [G.PlaneSpec("src", "in", 12, 21, np.uint8, 32, data=a, poison_rows=tuple(range(1, 12, 2))), G.PlaneSpec("dst", "out", 12, 21, np.uint8, 32)]

    def even_rows(arena):
        src, dst = _view(arena, "src"), _view(arena, "dst")
        seen.append(src[1::2, :21].copy())
        dst[::2, :21] = src[::2, :21]
        dst[1::2, :21] = src[::2, :21] + 1
    def exp2(specs):
        e = specs[0].data.copy()
        e[1::2] = e[::2] + 1
        return {"dst": e}
    G.run_case(G.NumpyBackend, make2, even_rows, exp2)
    assert (seen[0] == 0x00).all() and (seen[1] == 0xFF).all()

    def reads_them(arena):
        even_rows(arena)
        _view(arena, "dst")[3, 0] += _view(arena, "src")[3, 0] & 1
    with pytest.raises(G.FootprintError):
        G.run_case(G.NumpyBackend, make2, reads_them, exp2)


def test_guard_size_rule():
    a = G.Arena(G.NumpyBackend(), _specs()(), 0)
    assert a.guard == 4096
    wide = [G.PlaneSpec("src", "in", 4, 700, np.float32, 704, data=np.zeros((4, 700), np.float32))]
    b = G.Arena(G.NumpyBackend(), wide, 0xFF)
    assert b.guard == 8 * 704 * 4 and b.guard % 256 == 0
    assert b.specs[0].base == b.guard and b.nbytes == 2 * b.guard + 4 * 704 * 4
    assert (b.backend.copy_out()[:b.guard] == 0xFF).all()
