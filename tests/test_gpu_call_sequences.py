"""GPU: call SEQUENCES on one context - no result depends on what the context ran before.

Every other module checks a filter alone: upload (a synchronise), one call, download (another synchronise). A host queues many
different filters back to back on one context, and the context carries state from call to call: the shared
grow-only scratch buffer that every filter carves up differently, the clean-up protocols (who clears, who relies on the previous call
having cleaned up), the resident tables, the two internal streams and the buffers that grow by free-and-reallocate. Here the calls of a
case are all prepared first, then queued with no host synchronise in between (except where a call returns host scalars and therefore
synchronises by itself), then collected.

A recipe is one entry point on small planes:
    Recipe(seed, rng)   the host inputs (content from fx.splitmix64_plane and the filter modules' own constructions, seeded)
    prepare(dev)        uploads the inputs and allocates the outputs (both synchronise: all of them happen before the first queue())
    queue(dev)          the library call and nothing else
    collect(dev, ...)   downloads and compares with what the filter's own module compares with (oracle.* or tests/*_ref.py), by that
                        module's rule: pixels bit for bit (float included), integer scalars exact, SSIMULACRA2 abs = 1e-7
    release(dev)        frees what prepare() made besides planes
Expected values are computed once per (recipe, seed, sizes) and cached for the module."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

import bilateral_dither_ref as bd
import checkmate_ref as ck
import clahe_ref as clr
import color_map_ref as cm
import combmask_ref as cbr
import compress_ref as cpr
import fixtures as fx
import image_unpack_ref as iu
import mosquito_ref as mq
import pack_rgb_ref as pr
import test_gpu_bilateral_dither as tbd
import test_gpu_checkmate as tck
import test_gpu_color_map as tcm
import test_gpu_combmask as tcb
import test_gpu_compress as tcp
import test_gpu_deband as tdb
from oracle import vs_host as vh

pytestmark = pytest.mark.gpu
# soak runs: VSZIP_TEST_SEED_BASE=<n> shifts every seed of test_random_sequences (as in tests/test_gpu_random.py); the committed suite runs base 0
SEED_BASE = 100003 * int(os.environ.get("VSZIP_TEST_SEED_BASE", "0"))
SSIM_TOL = 1e-7  # tests/test_gpu_ssimulacra2.py
HANDOVER_PLANES = 256  # test_stream_handover: 1080p planes a call (1 GiB out, 2 GiB of scratch, about 1.5 ms a call); half as much did not show an unordered hand-over


@pytest.fixture(scope="module")
def dev():
    import vszip_amd

    d = vszip_amd.Device(0)
    yield d
    d.close()


def scratch_kib(dev) -> int:
    return dev.get_option("VSZIP_STAT_SCRATCH_KIB")


def _same(got, want) -> bool:
    """bit for bit (a float +0 is not a -0)"""
    want = np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint8), want.view(np.uint8))


def _differ(got, want) -> int:
    want = np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return -1
    return int((np.ascontiguousarray(got).view(np.uint8) != want.view(np.uint8)).sum())


_WANT = {}  # (recipe name, seed, sizes) -> expected value


class Recipe:
    name = ""
    stateful = False  # touches state that outlives the call (the table of the module's docstring)
    syncs = False     # returns host scalars, so the call synchronises by itself: queue() keeps the result

    def __init__(self, seed: int, rng=None):
        self.seed, self.got, self.key = int(seed), None, ()
        self.setup(rng)

    # -- the pieces a recipe fills in ----------------------------------------------------------------------------------------
    def setup(self, rng):
        raise NotImplementedError

    def expected(self, oracle):
        raise NotImplementedError

    def prepare(self, dev):
        raise NotImplementedError

    def queue(self, dev):
        raise NotImplementedError

    def release(self, dev):
        pass

    # -- shared ----------------------------------------------------------------------------------------------------------------
    def noise(self, i, shape, dtype):
        return fx.splitmix64_plane(self.seed * 4099 + 31 * i + 1, shape, dtype)

    @staticmethod
    def size(rng, default, lo, hi, even=False):
        """(h, w): the default, or drawn from lo .. hi (inclusive) per axis"""
        if rng is None:
            return default
        h, w = int(rng.integers(lo[0], hi[0] + 1)), int(rng.integers(lo[1], hi[1] + 1))
        return ((h // 2 * 2, w // 2 * 2) if even else (h, w))

    def want(self, oracle):
        k = (self.name, self.seed, self.key)
        if k not in _WANT:
            _WANT[k] = self.expected(oracle)
        return _WANT[k]

    def collect(self, dev, oracle, what=""):
        """pixel recipes: self.dsts against a list of planes"""
        want = self.want(oracle)
        assert len(want) == len(self.dsts)
        for i, (d, w) in enumerate(zip(self.dsts, want)):
            got = dev.download(d)
            assert _same(got, w), f"{what}: {self.name} seed {self.seed} plane {i} {w.shape} {w.dtype}: {_differ(got, w)} bytes differ"

    def up(self, dev, planes):
        return [dev.upload(np.ascontiguousarray(p)) for p in planes]

    def outs(self, dev, planes, dtype=None):
        return [dev.empty(p.shape[0], p.shape[1], dtype or p.dtype) for p in planes]


# ---- BoxBlur ------------------------------------------------------------------------------------------------------------------------
class _BoxBlur(Recipe):
    dtype, args, shapes = np.uint16, (5, 3, 5, 3), [(96, 160), (48, 80)]

    def setup(self, rng):
        self.key = (tuple(self.shapes), self.args)
        self.planes = [self.noise(i, s, self.dtype) for i, s in enumerate(self.shapes)]

    def expected(self, oracle):
        return [oracle.boxblur(p, *self.args) for p in self.planes]

    def prepare(self, dev):
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        dev.boxblur(self.srcs, self.dsts, *self.args)


class RtU16(_BoxBlur):
    """boxblur.hip: hpasses > 1 -> vszip_bb_rt. rt_plan: all three horizontal passes are one HSmall step (integer, radius <= kHsMaxR = 16),
    the three vertical passes are at least two steps (int_vspan: planes this short take chains of two), so run_rt has plan.size() >= 3 and
    its steps alternate between BOTH scratch plane sets."""
    name, stateful = "boxblur_rt_u16_3+3", True

    def setup(self, rng):
        h, w = self.size(rng, (96, 160), (40, 40), (96, 160))
        r = 5 if rng is None else int(rng.integers(1, 7))
        self.shapes, self.args = [(h, w), (h // 2, w // 2)], (r, 3, r, 3)
        super().setup(rng)


class RtBanded(_BoxBlur):
    """The shape and arguments of a call recorded in tests/rt_schedules.json ('chain in bands', u16, one plane of 136 x 50, vradius 9 x 3
    passes, default options), which tests/test_rt_plan_host.py holds rt_plan to: ichain_band_rows picks bands (two of 68 rows:
    boxblur_rt_ichain_kernel<u16, 2, 1> fills the per-column table that run_rt puts BEHIND the two plane sets, <u16, 2, 2> reads it), a
    vband pass follows - so 136 rows, more than the other recipes' 96: a band has at least 32 rows and a plane P (R + 1) + 1. The size
    is fixed: the path depends on it (test_recipes_are_on_their_paths)."""
    name, stateful = "boxblur_rt_int_banded", True
    shapes, args = [(136, 50)], (0, 0, 9, 3)


class RtF32(_BoxBlur):
    """float planes, 3 + 3 passes: rt_plan's float_span offers each axis as one chain; the vertical one qualifies (fchain_ok: the
    vertical float chain from one frame on), the horizontal passes go a launch each (rows < 12000) through both scratch plane sets."""
    name, stateful, dtype = "boxblur_rt_f32_3+3", True, np.float32

    def setup(self, rng):
        h, w = self.size(rng, (96, 160), (40, 40), (96, 160))
        r = 4 if rng is None else int(rng.integers(1, 7))
        self.shapes, self.args = [(h, w), (h // 2, w // 2)], (r, 3, r, 3)
        super().setup(rng)


class CtRing(_BoxBlur):
    """one pass each way, hradius == vradius <= 22: the compile-time-radius path (boxblur.hip: !use_rt), a width of whole 8-sample groups"""
    name = "boxblur_ct"

    def setup(self, rng):
        h, w = self.size(rng, (96, 160), (54, 48), (96, 160))
        r = 5 if rng is None else int(rng.integers(1, 12))
        self.shapes, self.args = [(h, (w + 7) // 8 * 8)], (r, 1, r, 1)
        super().setup(rng)


# ---- Bilateral ----------------------------------------------------------------------------------------------------------------------
class _Bilateral(Recipe):
    sig, kw = (2, 2), {}

    def setup(self, rng):
        self.shape = self.size(rng, (96, 160), (30, 30), (96, 160))
        self.key = (self.shape,)
        self.plane = self.noise(0, self.shape, np.uint16)

    def prepare(self, dev):
        self.cfg = dev.bilateral_cfg([self.sig[0]], [self.sig[1]], hist_len=65536, **self.kw)
        c = self.cfg[0]
        self.c = (c.sigmaS, c.sigmaR, c.algorithm, c.radius, c.step, c.pbficnum)
        self.check_path()
        self.srcs, self.dsts = self.up(dev, [self.plane]), self.outs(dev, [self.plane])

    def expected(self, oracle):
        return [oracle.bilateral_plane(self.plane, *self.c)]

    def queue(self, dev):
        dev.bilateral(self.srcs, self.dsts, self.cfg, [0])

    def release(self, dev):
        dev.bilateral_free(self.cfg)


class BilateralPbfic(_Bilateral):
    """algorithm = 1 (PBFIC + recursive Gaussian): bilateral.hip keeps the planes' `wj` layers at ctx->scratch (a.wj, offset 0)"""
    name, stateful = "bilateral_pbfic_u16", True
    sig, kw = (3, 0.1), dict(algorithm=[1], pbficnum=[4])

    def check_path(self):
        assert self.c[2] == 1 and self.c[5] == 4, self.c


class BilateralWalk(_Bilateral):
    """u16, no ref, sigmaS = 2 -> radius 3 / step 2 (the BASELINE's taps) and sigmaR = 2, whose range table packs: the column-walking kernel
    (launch_walk16<3, 2>; tests/test_gpu_bilateral.py::test_walk16_paths_agree runs this configuration) - its strip counter is ctx->scratch[0],
    cleared with hipMemsetAsync before every launch, its dummy store line lies 256 bytes behind"""
    name, stateful = "bilateral_walk_u16", True
    sig, kw = (2, 2), dict(algorithm=[2])

    def check_path(self):
        assert self.c[2:5] == (2, 3, 2), self.c


# ---- CLAHE --------------------------------------------------------------------------------------------------------------------------
class _Clahe(Recipe):
    dtype = np.uint16

    def setup(self, rng):
        h, w = self.size(rng, (96, 160), (24, 24), (96, 160))
        self.shapes = [(h, w), (max(h // 2, 3), max(w // 2, 3))]
        self.key = (tuple(self.shapes),)
        self.planes = [self.noise(i, s, self.dtype) for i, s in enumerate(self.shapes)]

    def expected(self, oracle):
        return [clr.clahe(p, 7, (3, 3)) for p in self.planes]

    def prepare(self, dev):
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        dev.clahe(self.srcs, self.dsts, 7, 3)


class ClaheU16(_Clahe):
    """tiles = 3: nine 65536-bin histograms a plane at the head of ctx->scratch (cleared per group with hipMemsetAsync), the LUTs behind them"""
    name, stateful = "clahe_u16", True


class ClaheU8(_Clahe):
    """the 8-bit form: 256-bin histograms, so the LUTs start where the 16-bit form keeps histogram bins"""
    name, stateful, dtype = "clahe_u8", True, np.uint8


# ---- Deband -------------------------------------------------------------------------------------------------------------------------
class _Deband7(Recipe):
    """sample_mode = 7: deband.hip computes the planes' angle planes into ctx->scratch first, the sampling kernel reads them"""
    dtype = np.uint16
    SIZES = [[(45, 131), (40, 97)], [(31, 64), (45, 131)], [(40, 97)]]  # (the tables are made per size: a few sizes, shared with the other tests)

    def setup(self, rng):
        self.shapes = self.SIZES[0] if rng is None else self.SIZES[int(rng.integers(0, len(self.SIZES)))]
        self.key = (tuple(self.shapes),)
        f = np.dtype(self.dtype) == np.float32
        self.items = []
        for k, (h, w) in enumerate(self.shapes):
            t = tdb.tables(w, h, 7, f)
            self.items.append(tdb.item(tdb.plane(3 + self.seed * 5 + k, h, w, self.dtype), t, grain=t["grain_y"]))

    def expected(self, oracle):
        return [tdb.expected(it, 7) for it in self.items]

    def prepare(self, dev):
        up = {}

        def resident(a, as_pairs):  # (tests/test_gpu_deband.py::run)
            if id(a) not in up:
                up[id(a)] = dev.upload(np.ascontiguousarray(a).view(np.int16).reshape(a.shape[0], a.shape[1]) if as_pairs else a.reshape(1, -1))
            return up[id(a)]
        self.srcs = [dev.upload(it["src"]) for it in self.items]
        self.dsts = [dev.empty(it["src"].shape[0], it["src"].shape[1], it["src"].dtype) for it in self.items]
        self.entries = [dev.deband_entry(resident(it["table"], True), it["ssw"], it["ssh"], resident(it["grain"], False), it["goff"], it["gpitch"], *it["thr"], it["lo"], it["hi"])
                        for it in self.items]
        self.tables = up

    def queue(self, dev):
        dev.deband(self.srcs, self.dsts, self.entries, 7, True, 1.5, 0.15, 15)


class Deband7U16(_Deband7):
    name, stateful = "deband_mode7_u16", True


class Deband7F32(_Deband7):
    name, stateful, dtype = "deband_mode7_f32", True, np.float32


# ---- EEDI3 --------------------------------------------------------------------------------------------------------------------------
class Eedi3Fork(Recipe):
    """vcheck = 2 on one tall and two short planes (a 4:2:0 frame) in one call: eedi3.hip `split` - the tuned line kernel (mdis <= 20), the
    LDS consistency chains (lines <= kVcLdsMaxL), 0 < tall planes < planes - runs the short planes' line kernel on ctx->aux_stream beside
    the tall planes' chains, forked with aux_fork and joined with aux_join. The library does so from 12 tall planes on; the call sets
    VSZIP_EEDI3_FORCE_OVERLAP like tests/test_gpu_eedi3.py::test_two_plane_heights_overlap_equals_sequential_and_oracle. The DP tables of
    all lines are in ctx->scratch."""
    name, stateful = "eedi3_vcheck2_fork", True
    KW = dict(vcheck=2, mdis=10, nrad=2)

    def setup(self, rng):
        h, w = self.size(rng, (64, 128), (24, 64), (64, 128), even=True)
        self.shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        if (h // 2) % 2:
            self.shapes = [(h + 2, w), (h // 2 + 1, w // 2), (h // 2 + 1, w // 2)]
        self.key = (tuple(self.shapes),)
        self.planes = [self.noise(i, s, np.float32) for i, s in enumerate(self.shapes)]

    def expected(self, oracle):
        return [oracle.eedi3(p, 1, **self.KW) for p in self.planes]

    def prepare(self, dev):
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        with dev.options(VSZIP_EEDI3_FORCE_OVERLAP=1):  # (host state only: nothing is queued or awaited)
            dev.eedi3_into(self.srcs, self.dsts, 1, **self.KW)


# ---- plane statistics -----------------------------------------------------------------------------------------------------------------
class _Stats(Recipe):
    syncs = True

    def setup(self, rng):
        h, w = self.size(rng, (96, 160), (8, 16), (96, 160))
        self.shapes = [(h, w), (max(h // 2, 1), max(w // 2, 1))]
        self.key = (tuple(self.shapes),)
        self.planes = [self.noise(i, s, np.uint16) for i, s in enumerate(self.shapes)]
        for p in self.planes:
            p[::3, ::5] = 100
        self.refs = [self.noise(10 + i, s, np.uint16) for i, s in enumerate(self.shapes)]

    def prepare(self, dev):
        self.srcs, self.drefs = self.up(dev, self.planes), self.up(dev, self.refs)

    def collect(self, dev, oracle, what=""):
        assert self.got == self.want(oracle), f"{what}: {self.name} seed {self.seed} {self.shapes}: {self.got} != {self.want(oracle)}"


class PlaneAverage(_Stats):
    """exclude and refs: planestats.hip keeps the per-block partial sums (sum, count, difference) at the head of ctx->scratch and returns through
    ctx->scalars_host. (Integer planes: the averages are exact, tests/test_gpu_planestats.py.) Synchronises by itself."""
    name, stateful = "plane_average_exclude_refs", True
    EXCL = [100, 7]

    def expected(self, oracle):
        r = [oracle.plane_average(a, self.EXCL, b) for a, b in zip(self.planes, self.refs)]
        return ([x[0] for x in r], [x[1] for x in r])

    def queue(self, dev):
        self.got = dev.plane_average(self.srcs, self.EXCL, self.drefs)


class PlaneMinMax(_Stats):
    """thresholds > 0 on u16 planes: the histogram sweeps (histograms and buckets in ctx->scratch, cleared with hipMemsetAsync), the
    per-plane prediction tables (ctx->minmax_pred: a call of the previous call's shape looks where that one's answers lay) and
    ctx->scalars_host. Synchronises by itself."""
    name, stateful = "plane_minmax_thr_u16", True

    def expected(self, oracle):
        r = [oracle.plane_minmax(a, 0.1, 0.1, b) for a, b in zip(self.planes, self.refs)]
        return ([x[0] for x in r], [x[1] for x in r], [x[2] for x in r])

    def queue(self, dev):
        self.got = dev.plane_minmax(self.srcs, 0.1, 0.1, self.drefs)


# ---- XPSNR --------------------------------------------------------------------------------------------------------------------------
class _Xpsnr(Recipe):
    syncs, nf, fps = True, 1, 24

    def setup(self, rng):
        h, w = self.size(rng, self.default, (32, 32), self.default, even=True)
        self.shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        self.key = (tuple(self.shapes),)
        n = self.nf + 2  # two frames before the first: prev1 / prev2 of every frame exist
        self.frames = [[self.noise(3 * f + i, s, np.uint8) for i, s in enumerate(self.shapes)] for f in range(n)]
        self.recs = [[np.clip(p.astype(np.int32) + (self.noise(100 + 3 * f + i, p.shape, np.uint8) % 13).astype(np.int32) - 6, 0, 255).astype(np.uint8) for i, p in enumerate(fr)]
                     for f, fr in enumerate(self.frames)]

    def expected(self, oracle):
        # (the frame before the previous one is read from 32 fps on: tests/test_gpu_xpsnr.py)
        return [oracle.xpsnr_wsse(self.frames[f], self.recs[f], self.frames[f - 1][0], self.frames[f - 2][0] if self.fps >= 32 else None, depth=8, frame_rate=self.fps)
                for f in range(2, self.nf + 2)]

    def prepare(self, dev):
        self.dfr = [self.up(dev, fr) for fr in self.frames]
        self.drc = [self.up(dev, fr) for fr in self.recs[2:]]

    def collect(self, dev, oracle, what=""):
        assert self.got == self.want(oracle), f"{what}: {self.name} seed {self.seed} {self.shapes}: {self.got} != {self.want(oracle)}"


class XpsnrOne(_Xpsnr):
    """one frame: the block sums accumulate in ctx->xpsnr_sums, which the weighting kernel leaves zeroed for the next call
    (ctx->xpsnr_clean: no memset while it holds); the result comes through ctx->scalars_host. Synchronises by itself."""
    name, stateful, default = "xpsnr_one_frame", True, (96, 160)

    def queue(self, dev):
        self.got = [dev.xpsnr_wsse(self.dfr[2], self.drc[0], self.dfr[1][0], None, depth=8, frame_rate=self.fps)]


class XpsnrBatch9(_Xpsnr):
    """nine frames, one more than kInlineFrames = 8 (xpsnr.hip): the frame table no longer fits the kernel arguments - it is written into
    ctx->scalars_host and copied to ctx->scratch, where the strip kernel reads it. 60 fps: both previous frames are read. Synchronises by itself."""
    name, stateful, default, nf, fps = "xpsnr_batch_9", True, (48, 64), 9, 60

    def queue(self, dev):
        nf = self.nf
        p1 = [self.dfr[f + 1][0] for f in range(nf)]
        p2 = [self.dfr[f][0] for f in range(nf)]
        self.got = dev.xpsnr_wsse_batch(self.dfr[2:], self.drc, p1, p2, depth=8, frame_rate=self.fps)


# ---- SSIMULACRA2 --------------------------------------------------------------------------------------------------------------------
class _Ssim(Recipe):
    syncs = True

    def collect(self, dev, oracle, what=""):
        assert self.got == pytest.approx(self.want(oracle), abs=SSIM_TOL), f"{what}: {self.name} seed {self.seed} {self.key}: {self.got} != {self.want(oracle)}"


class SsimRgbs(_Ssim):
    """linear RGBS: the pyramid and the maps' partial sums in ctx->scratch, the pointer tables and the averages in ctx->scalars_host, the
    small scales on ctx->side_stream (ssimulacra2.hip `two`: every call unless VSZIP_SSIM_ONE_STREAM), joined before the final reduction.
    Synchronises by itself."""
    name, stateful = "ssimulacra2_rgbs", True

    def setup(self, rng):
        self.shape = self.size(rng, (64, 96), (16, 16), (64, 96))
        self.key = (self.shape,)
        self.ref = [self.noise(i, self.shape, np.float32) for i in range(3)]
        self.dis = [np.clip(p + (self.noise(10 + i, self.shape, np.float32) - np.float32(0.5)) * np.float32(0.1), 0, 1).astype(np.float32) for i, p in enumerate(self.ref)]

    def expected(self, oracle):
        return oracle.ssimulacra2(self.ref, self.dis)

    def prepare(self, dev):
        self.dr, self.dd = [dev.upload(p, 1) for p in self.ref], [dev.upload(p, 1) for p in self.dis]

    def queue(self, dev):
        self.got = dev.ssimulacra2(self.dr, self.dd)[0]


def _yuv420p8(recipe, shape, base=0):
    h, w = shape
    lo, hi = 16, 235
    y = (lo + recipe.noise(base, (h, w), np.uint8).astype(np.int32) * (hi - lo) // 255).astype(np.uint8)
    return [y, recipe.noise(base + 1, (h // 2, w // 2), np.uint8), recipe.noise(base + 2, (h // 2, w // 2), np.uint8)]


def _yuv_linear(planes):
    return [vh.srgb_to_linear(p) for p in vh.yuv_to_rgbs(planes, 8, 1, 1, 1, 0, limited=True)]


class SsimYuv(_Ssim):
    """from YUV420P8 (vszip_ssimulacra2_src): the colour pre-stage reads its conversion table from the cache at ctx->ssim_lut, built on
    the first call of a format and reused by every later one. Synchronises by itself."""
    name, stateful = "ssimulacra2_yuv420p8", True

    def setup(self, rng):
        self.shape = self.size(rng, (64, 96), (16, 16), (64, 96), even=True)
        self.key = (self.shape,)
        self.ref = _yuv420p8(self, self.shape)
        self.dis = [np.clip(p.astype(np.int32) + (self.noise(20 + i, p.shape, np.uint8) % 9).astype(np.int32) - 4, 0, 255).astype(np.uint8) for i, p in enumerate(self.ref)]

    def expected(self, oracle):
        return oracle.ssimulacra2(_yuv_linear(self.ref), _yuv_linear(self.dis))

    def prepare(self, dev):
        self.fmt = dev.ssim_source("YUV", np.uint8, 8, True, limited=True, ssw=1, ssh=1, matrix=1, chroma_loc=0)
        self.dr, self.dd = self.up(dev, self.ref), self.up(dev, self.dis)

    def queue(self, dev):
        self.got = dev.ssimulacra2_src(self.fmt, self.dr, self.dd)[0]


class ToRgbs(Recipe):
    name = "to_rgbs_linear"

    def setup(self, rng):
        self.shape = self.size(rng, (64, 96), (8, 8), (64, 96), even=True)
        self.key = (self.shape,)
        self.planes = _yuv420p8(self, self.shape)

    def expected(self, oracle):
        return _yuv_linear(self.planes)

    def prepare(self, dev):
        self.fmt = dev.ssim_source("YUV", np.uint8, 8, True, limited=True, ssw=1, ssh=1, matrix=1, chroma_loc=0)
        self.srcs = self.up(dev, self.planes)
        self.dsts = [dev.empty(self.shape[0], self.shape[1], np.float32) for _ in range(3)]

    def queue(self, dev):
        dev.to_rgbs_linear_into(self.fmt, self.srcs, self.dsts)


# ---- the point filters ----------------------------------------------------------------------------------------------------------------
class _Point(Recipe):
    dtype = np.uint16

    def setup(self, rng):
        h, w = self.size(rng, (67, 131), (1, 1), (96, 160))
        self.shapes = [(h, w), (max(h // 2, 1), max(w // 2, 1))]
        self.key = (tuple(self.shapes),)
        self.planes = [self.noise(i, s, self.dtype) for i, s in enumerate(self.shapes)]
        self.others = [self.noise(10 + i, s, self.dtype) for i, s in enumerate(self.shapes)]

    def prepare(self, dev):
        self.srcs, self.dothers, self.dsts = self.up(dev, self.planes), self.up(dev, self.others), self.outs(dev, self.planes)


class Limiter(_Point):
    name, LO, HI = "limiter", [4096.0, 8000.0], [60160.0, 30000.0]

    def expected(self, oracle):
        return [oracle.limiter(p, lo, hi) for p, lo, hi in zip(self.planes, self.LO, self.HI)]

    def queue(self, dev):
        dev.limiter(self.srcs, self.dsts, self.LO, self.HI)


class LimitFilter(_Point):
    name, DARK, BRIGHT, ELAST = "limit_filter", [900.0, 300.0], [1200.0, 500.0], [2.0, 1.5]

    def expected(self, oracle):
        return [oracle.limit_filter(f, s, None, np.float32(d), np.float32(b), np.float32(e)) for f, s, d, b, e in zip(self.planes, self.others, self.DARK, self.BRIGHT, self.ELAST)]

    def queue(self, dev):
        dev.limit_filter(self.srcs, self.dothers, self.dsts, self.DARK, self.BRIGHT, self.ELAST)


class AdaptiveBinarize(_Point):
    name, dtype = "adaptive_binarize", np.uint8

    def setup(self, rng):
        super().setup(rng)
        self.others = [np.clip(p.astype(np.int16) + (o % 13).astype(np.int16) - 6, 0, 255).astype(np.uint8) for p, o in zip(self.planes, self.others)]

    def expected(self, oracle):
        return [oracle.adaptive_binarize(a, b, 3) for a, b in zip(self.planes, self.others)]

    def queue(self, dev):
        dev.adaptive_binarize(self.srcs, self.dothers, self.dsts, 3)


# ---- the eleven filters of the C ABI that the plugin does not have --------------------------------------------------------------------
class _Comb(Recipe):
    def setup(self, rng):
        self.shape = self.size(rng, (67, 131), (3, 1), (96, 160))
        self.key = (self.shape,)
        self.cur, self.prev = tcb._combed(self.seed, self.shape)

    def prepare(self, dev):
        self.srcs, self.dprev, self.dsts = self.up(dev, [self.cur]), self.up(dev, [self.prev]), self.outs(dev, [self.cur])


class CombMask(_Comb):
    name = "comb_mask"

    def expected(self, oracle):
        return [cbr.comb_mask(self.cur, self.prev, cthresh=6, mthresh=9, expand=True, metric=0)]

    def queue(self, dev):
        dev.comb_mask(self.srcs, self.dsts, self.dprev, cthresh=6, mthresh=9, expand=True, metric=0)


class CombMaskMT(_Comb):
    name = "comb_mask_mt"

    def expected(self, oracle):
        return [cbr.comb_mask_mt(self.cur, 30, 30)]

    def queue(self, dev):
        dev.comb_mask_mt(self.srcs, self.dsts, 30, 30)


class Checkmate(Recipe):
    name = "checkmate"

    def setup(self, rng):
        self.shape = self.size(rng, (40, 131), (5, 3), (70, 160))
        self.key = (self.shape,)
        self.set = tck.correlated(self.seed * 7 + 1, self.shape)  # p2, p1, cur, n1, n2

    def expected(self, oracle):
        return [ck.checkmate(*self.set, thr=12, tmax=12, tthr2=8)]

    def prepare(self, dev):
        self.d = self.up(dev, self.set)
        self.dsts = self.outs(dev, [self.set[2]])

    def queue(self, dev):
        p2, p1, cur, n1, n2 = self.d
        dev.checkmate([cur], self.dsts, [p1], [n1], [p2], [n2], thr=12, tmax=12, tthr2=8)


class Mosquito(Recipe):
    name = "mosquito_nr"

    def setup(self, rng):
        self.shape = self.size(rng, (45, 99), (4, 4), (70, 131))
        self.key = (self.shape,)
        self.planes = [self.noise(0, self.shape, np.uint16)]

    def expected(self, oracle):
        return [mq.mosquito_nr(p, 16, 128, 2, 16, False) for p in self.planes]

    def prepare(self, dev):
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        dev.mosquito_nr(self.srcs, self.dsts, 16, 128, 2, 16, None)


class BilateralDither(Recipe):
    name = "bilateral_dither"

    def setup(self, rng):
        self.shape = self.size(rng, (45, 67), (16, 16), (45, 99))
        self.key = (self.shape,)
        self.items = [tbd.item(bd.noisy_plane(3 + self.seed, self.shape[0], self.shape[1], np.uint16), subspl=2.0)]

    def expected(self, oracle):
        return [bd.plane(it["src"], it["radius"], it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], it["bits"], it["pts"], it["ref"]) for it in self.items]

    def prepare(self, dev):  # (tests/test_gpu_bilateral_dither.py::run, the dense window: no point lists)
        self.srcs = [dev.upload(it["src"]) for it in self.items]
        self.dsts = [dev.empty(it["src"].shape[0], it["src"].shape[1], it["src"].dtype) for it in self.items]
        assert all(it["pts"] is None for it in self.items)
        self.entries = [dev.bilateral_dither_entry(it["radius"], it["d"]["m"], it["d"]["wmax"], it["d"]["sum_w_min"], None, it["d"]["K"]) for it in self.items]

    def queue(self, dev):
        dev.bilateral_dither(self.srcs, self.dsts, self.entries, None, self.items[0]["bits"])


class Compress(Recipe):
    name = "compress"

    def setup(self, rng):
        self.shape = self.size(rng, (67, 130), (1, 1), (83, 130))
        self.key = (self.shape,)
        self.planes = [cpr.gpu_plane(self.seed, self.shape[1], self.shape[0])]

    def expected(self, oracle):
        return [cpr.plane(p, cpr.tables(**cpr.DEFAULTS), False) for p in self.planes]

    def prepare(self, dev):
        self.tables = tcp.lib_tables({})
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        dev.compress(self.srcs, self.dsts, self.tables, None)


class PackRGB(Recipe):
    name = "pack_rgb"

    def setup(self, rng):
        self.shape = self.size(rng, (37, 257), (1, 1), (40, 300))
        self.key = (self.shape,)
        self.frame = pr.gpu_frame(self.seed, self.shape[1], self.shape[0], 8)

    def expected(self, oracle):
        return [pr.pack(*self.frame, 8)]

    def prepare(self, dev):
        self.d = self.up(dev, self.frame)
        self.dsts = [dev.empty(self.shape[0], self.shape[1], np.uint32)]

    def queue(self, dev):
        dev.pack_rgb([self.d[0]], [self.d[1]], [self.d[2]], self.dsts, 8)


class ColorMap(Recipe):
    name = "color_map"

    def setup(self, rng):
        self.shape = self.size(rng, (37, 257), (1, 1), (40, 300))
        self.key = (self.shape,)
        self.plane = cm.gpu_plane(self.seed, self.shape[1], self.shape[0])

    def expected(self, oracle):
        return list(cm.apply(self.plane, tcm.LUT))

    def prepare(self, dev):
        self.srcs = self.up(dev, [self.plane])
        self.dsts = [dev.empty(self.shape[0], self.shape[1], np.uint8) for _ in range(3)]

    def queue(self, dev):
        dev.color_map(self.srcs, [self.dsts[0]], [self.dsts[1]], [self.dsts[2]], tcm.LUT)


class ImageUnpack(Recipe):
    name, COMBO = "image_unpack", (iu.RGBA, np.uint8, 8)

    def setup(self, rng):
        self.shape = self.size(rng, (37, 83), (1, 1), (40, 131))
        self.key = (self.shape,)
        self.packed = iu.content(self.seed, self.shape[0], self.shape[1], self.COMBO)

    def expected(self, oracle):
        colour, alpha = iu.unpack(self.packed, self.COMBO[0], self.COMBO[2], None)
        return list(colour) + [alpha]

    def prepare(self, dev):
        self.srcs = self.up(dev, [iu.row_bytes(self.packed)])
        self.dsts = [dev.empty(self.shape[0], self.shape[1], np.uint8) for _ in range(4)]

    def queue(self, dev):
        dev.image_unpack(self.srcs, [self.dsts[:3]], [self.dsts[3]], self.COMBO[0], self.COMBO[2], None)


class ChainRun(Recipe):
    """vszip_chain_run: a BoxBlur stage into the context's ctx->chain_buf, a Limiter stage from there"""
    name, LO, HI = "chain_run", [4096.0, 8000.0, 8000.0], [60160.0, 50000.0, 50000.0]

    def setup(self, rng):
        h, w = self.size(rng, (64, 96), (16, 16), (64, 96), even=True)
        self.shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        self.key = (tuple(self.shapes),)
        self.planes = [self.noise(i, s, np.uint16) for i, s in enumerate(self.shapes)]

    def expected(self, oracle):
        return [oracle.limiter(oracle.boxblur(p, 3, 1, 3, 1), self.LO[i], self.HI[i]) for i, p in enumerate(self.planes)]

    def prepare(self, dev):
        self.srcs, self.dsts = self.up(dev, self.planes), self.outs(dev, self.planes)

    def queue(self, dev):
        dev.chain_run([{"boxblur": (3, 1, 3, 1)}, {"limiter": (self.LO, self.HI)}], self.srcs, self.dsts, [0, 1, 2])


STATEFUL = [RtU16, RtBanded, RtF32, BilateralPbfic, BilateralWalk, ClaheU16, ClaheU8, Deband7U16, Deband7F32, Eedi3Fork, PlaneAverage, PlaneMinMax, XpsnrOne, XpsnrBatch9,
            SsimRgbs, SsimYuv]
PLAIN = [CtRing, Limiter, LimitFilter, AdaptiveBinarize, CombMask, CombMaskMT, Checkmate, Mosquito, BilateralDither, Compress, PackRGB, ColorMap, ImageUnpack, ChainRun, ToRgbs]
ALL = STATEFUL + PLAIN
assert all(r.stateful for r in STATEFUL) and not any(r.stateful for r in PLAIN) and len({r.name for r in ALL}) == len(ALL)
_ids = lambda rs: [r.name for r in rs]


def run_sequence(dev, oracle, jobs, what=""):
    """prepare all (uploads synchronise), queue all back to back, collect all"""
    for j in jobs:
        j.prepare(dev)
    try:
        for j in jobs:
            j.queue(dev)
        for i, j in enumerate(jobs):
            j.collect(dev, oracle, f"{what} step {i}")
    finally:
        dev.sync()
        for j in jobs:
            j.release(dev)


# ---- the filler: a call that leaves the scratch buffer full of 0xFF ---------------------------------------------------------------------
class Filler:
    """RT BoxBlur 3 + 3 on u16 planes of 0xFFFF: every intermediate is 0xFFFF, so the two scratch plane sets it goes through - the head of
    ctx->scratch, 2 x 4 x 1080 x 1920 samples = 31.6 MiB - are all 0xFF bytes afterwards: NaN to whoever reads floats there, -1 or 4 G to
    whoever reads a counter or a histogram bin. (A scratch pitch is the width rounded up to 64 samples: 1920 is whole, no byte is left out.)"""
    SHAPE, N, ARGS = (1080, 1920), 4, (5, 3, 5, 3)

    def __init__(self, dev):
        full = np.full(self.SHAPE, 0xFFFF, np.uint16)
        self.srcs = [dev.upload(full) for _ in range(self.N)]
        self.dsts = [dev.empty(self.SHAPE[0], self.SHAPE[1], np.uint16) for _ in range(self.N)]

    def queue(self, dev):
        for d in self.dsts:
            dev.check(dev.lib.vszip_dev_memset(dev.ctx, d.ptr, 0, d.nbytes))  # (on the stream, before the call: a call that wrote nothing would be seen)
        dev.boxblur(self.srcs, self.dsts, *self.ARGS)

    def collect(self, dev, what=""):
        for i, d in enumerate(self.dsts):
            got = dev.download(d)
            assert int(got.min()) == 0xFFFF, f"{what}: the filler's plane {i} has {int((got != 0xFFFF).sum())} samples that are not 0xFFFF"


@pytest.fixture(scope="module")
def filler(dev):
    f = Filler(dev)
    f.queue(dev)  # sizes the buffer
    f.collect(dev, "sizing run")
    print("scratch KiB after the filler:", scratch_kib(dev))
    return f


@pytest.fixture(scope="module")
def needs():
    """what each stateful recipe asks of the scratch buffer, measured on a fresh context each: VSZIP_STAT_SCRATCH_KIB after the call alone
    (an allocation is the request + 1/8 + 4 KiB, the filler's like the recipes')"""
    import vszip_amd

    out = {}
    for R in STATEFUL:
        d = vszip_amd.Device(0)
        j = R(0)
        j.prepare(d)
        j.queue(d)
        d.sync()
        out[R.name] = scratch_kib(d)
        j.release(d)
        del j
        d.close()
    return out


def test_recipes_are_on_their_paths(dev, needs):
    """what can be shown about the paths the stateful recipes' comments name"""
    # the banded chain: the recipe IS a recorded call whose launches are the banded chain's two kernels (tests/test_rt_plan_host.py ties rt_plan to the record)
    rec = json.loads((Path(__file__).resolve().parent / "rt_schedules.json").read_text())["calls"]
    j = RtBanded(0)
    j.prepare(dev)
    plane = [j.shapes[0][0], j.shapes[0][1], j.srcs[0].stride, j.dsts[0].stride, (j.srcs[0].ptr | j.srcs[0].stride * 2) & 15, (j.dsts[0].ptr | j.dsts[0].stride * 2) & 15]
    hits = [c for c in rec if c["dtype"] == "u16" and c["frames"] == 1 and c["planes"] == [plane] and tuple(c["args"]) == j.args and c["options"] == {}]
    assert len(hits) == 1, plane
    names = [k[0] for k in hits[0]["kernels"]]
    assert "boxblur_rt_ichain_kernel<u16, 2, 1>" in names and "boxblur_rt_ichain_kernel<u16, 2, 2>" in names, names
    # every stateful recipe but one keeps something in the scratch buffer (the Bilateral walk kernel: its 512 bytes)
    print("scratch KiB by recipe:", needs)
    for R in STATEFUL:
        assert (needs[R.name] > 0) == (R is not XpsnrOne), R.name  # (a single XPSNR frame keeps its state in ctx->xpsnr_sums, not in the scratch buffer)
    # thresholded PlaneMinMax: the second call of a shape runs the predicted sweep from the table the first one left
    a, b = PlaneMinMax(0), PlaneMinMax(0)
    a.prepare(dev)
    b.prepare(dev)
    a.queue(dev)
    before = dev.get_option("VSZIP_STAT_MINMAX_PREDICTED")
    b.queue(dev)
    assert dev.get_option("VSZIP_STAT_MINMAX_PREDICTED") > before
    assert a.got == b.got


@pytest.mark.parametrize("R", STATEFUL, ids=_ids(STATEFUL))
def test_after_dirty_scratch(dev, oracle, filler, needs, R):
    """the recipe right behind the filler, in the buffer the filler dirtied: a kernel that reads a scratch word before writing it, or a
    clear that is short, reads 0xFF bytes here (fresh from hipMalloc, as in every other module, they are zero in practice)"""
    kib_sized = scratch_kib(dev)
    assert kib_sized > max(needs.values()), (kib_sized, needs)  # no recipe makes the buffer grow: it runs where the filler ran
    j = R(0)
    j.prepare(dev)
    try:
        filler.queue(dev)
        kib = scratch_kib(dev)
        j.queue(dev)  # (no dev.sync() in between)
        j.collect(dev, oracle, "behind the filler")
        filler.collect(dev, f"before {R.name}")
        assert scratch_kib(dev) == kib == kib_sized, "the scratch buffer was reallocated: the case proved nothing"
    finally:
        dev.sync()
        j.release(dev)


@pytest.mark.parametrize("A", STATEFUL, ids=_ids(STATEFUL))
def test_ordered_pairs(dev, oracle, A):
    """A then B for every stateful B (A itself included, on other content): what A leaves - scratch bytes, a clean-up flag, a prediction, a
    cached table, a forked stream - must not reach B's result. Where A returns host scalars (plane statistics, XPSNR, SSIMULACRA2: `syncs`) its
    call synchronises by itself, and the pair checks what a FINISHED A leaves; the others are still running when B is queued."""
    for B in STATEFUL:
        run_sequence(dev, oracle, [A(0), B(1)], f"{A.name} -> {B.name}")


def test_output_consumed_without_sync(dev, oracle):
    """the next call reads a previous call's destination with no host synchronise in between; expected: the oracle's composition"""
    # EEDI3 (forked onto the aux stream: the short planes' lines are written there) -> BoxBlur on its dst: what aux_join is for
    e = Eedi3Fork(2)
    e.prepare(dev)
    blurred = e.outs(dev, e.planes)
    e.queue(dev)
    dev.boxblur(e.dsts, blurred, 2, 1, 2, 1)
    for i, (d, w) in enumerate(zip(blurred, e.want(oracle))):
        assert _same(dev.download(d), oracle.boxblur(w, 2, 1, 2, 1)), ("eedi3 -> boxblur", i)
    e.collect(dev, oracle, "eedi3 -> boxblur")

    # to_rgbs_linear (twice) -> SSIMULACRA2 on its outputs
    s = SsimYuv(2)
    s.prepare(dev)
    rgb = [[dev.empty(s.shape[0], s.shape[1], np.float32) for _ in range(3)] for _ in range(2)]
    dev.to_rgbs_linear_into(s.fmt, s.dr, rgb[0])
    dev.to_rgbs_linear_into(s.fmt, s.dd, rgb[1])
    got = dev.ssimulacra2(rgb[0], rgb[1])[0]
    assert got == pytest.approx(s.want(oracle), abs=SSIM_TOL), "to_rgbs_linear -> ssimulacra2"

    # Deband mode 7 -> Limiter
    d7 = Deband7U16(2)
    d7.prepare(dev)
    lim = d7.outs(dev, [it["src"] for it in d7.items])
    lo, hi = [9000.0] * len(lim), [40000.0] * len(lim)
    d7.queue(dev)
    dev.limiter(d7.dsts, lim, lo, hi)
    for i, (d, w) in enumerate(zip(lim, d7.want(oracle))):
        assert _same(dev.download(d), oracle.limiter(w, lo[i], hi[i])), ("deband -> limiter", i)

    # CLAHE -> PlaneMinMax (synchronises by itself: it returns the answers)
    c = ClaheU16(2)
    c.prepare(dev)
    c.queue(dev)
    mn, mx, _ = dev.plane_minmax(c.dsts, 0.1, 0.1)
    for i, w in enumerate(c.want(oracle)):
        assert (mn[i], mx[i]) == oracle.plane_minmax(w, 0.1, 0.1)[:2], ("clahe -> plane_minmax", i)

    # BoxBlur RT -> XPSNR with the blur as `rec`
    x = XpsnrOne(2)
    x.prepare(dev)
    org = x.dfr[2]
    rec = x.outs(dev, x.frames[2])
    dev.boxblur(org, rec, 2, 2, 2, 2)
    got = dev.xpsnr_wsse(org, rec, x.dfr[1][0], None, depth=8, frame_rate=24)
    assert got == oracle.xpsnr_wsse(x.frames[2], [oracle.boxblur(p, 2, 2, 2, 2) for p in x.frames[2]], x.frames[1][0], None, depth=8, frame_rate=24), "boxblur -> xpsnr"


def test_scratch_grows_mid_queue(oracle):
    """vszip_ensure_scratch / vszip_ensure_scalars grow by synchronise, free and reallocate, in the middle of whatever is queued"""
    import vszip_amd

    d = vszip_amd.Device(0)
    try:
        small, large, again = ClaheU8(3), ClaheU16(3), ClaheU8(4)  # 18 histograms of 256 bins, then of 65536, then of 256 again
        for j in (small, large, again):
            j.prepare(d)
        small.queue(d)
        kib = scratch_kib(d)
        large.queue(d)
        assert scratch_kib(d) > kib > 0
        again.queue(d)
        for j in (small, large, again):
            j.collect(d, oracle, "scratch grows")
        # scalars_host: PlaneAverage on 3 planes (one 4 KiB page), on 300 (9600 bytes: three pages), on 3 again
        planes = [fx.splitmix64_plane(900 + i, (8 + i % 5, 16 + i % 7), np.uint16) for i in range(300)]
        dp = [d.upload(p) for p in planes]
        for sel in (range(3), range(300), range(297, 300)):
            avg, _ = d.plane_average([dp[i] for i in sel], [7])
            assert avg == [oracle.plane_average(planes[i], [7])[0] for i in sel], len(sel)
    finally:
        d.close()


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences(dev, oracle, seed):
    """10 .. 14 calls drawn from all recipes, fresh content and sizes per step, queued back to back, collected at the end"""
    s = SEED_BASE + 11000 + seed
    rng = np.random.default_rng(s)
    kinds = [ALL[int(k)] for k in rng.integers(0, len(ALL), size=int(rng.integers(10, 15)))]
    jobs = [R(s * 16 + step, rng) for step, R in enumerate(kinds)]
    run_sequence(dev, oracle, jobs, f"seed {s}: {[R.name for R in kinds]}")


def test_stream_handover(oracle):
    """vszip_ctx_set_stream from one caller's stream to another (a PyTorch host following torch.cuda.current_stream()): what the context
    queued on the first stream is ordered before what it queues on the second (include/vszip_hip.h). A and B are the same RT BoxBlur on the
    same shapes, so both use the same bytes of ctx->scratch for their intermediates: unordered, B's passes overwrite the planes A's passes
    are still reading.
    Against the library as it was before the rule (no ordering in vszip_ctx_set_stream) this test passed with 512 planes of 540 x 960 a call
    and failed with HANDOVER_PLANES = 256 planes of 1080p: all 256 planes of call A differed from the oracle."""
    import torch

    import vszip_amd

    shape, n, args = (1080, 1920), HANDOVER_PLANES, (5, 3, 5, 3)
    d = vszip_amd.Device(0)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        calls = []
        for c in range(2):  # every upload first: uploads run and synchronise on the context's own stream
            content = [fx.splitmix64_plane(500 + 10 * c + k, shape, np.uint16) for k in range(2)]
            srcs = [d.upload(p) for p in content]
            calls.append((content, [srcs[k % 2] for k in range(n)], [d.empty(shape[0], shape[1], np.uint16) for _ in range(n)]))
        d.set_stream(s1.cuda_stream)
        d.boxblur(calls[0][1], calls[0][2], *args)
        d.set_stream(s2.cuda_stream)
        d.boxblur(calls[1][1], calls[1][2], *args)
        s1.synchronize()
        s2.synchronize()
        for c, (content, _, dsts) in enumerate(calls):
            want = [oracle.boxblur(p, *args) for p in content]
            bad = [k for k, o in enumerate(dsts) if not np.array_equal(d.download(o), want[k % 2])]
            assert not bad, f"call {'AB'[c]}: {len(bad)} of {n} planes differ from the oracle, the first {bad[:8]}"
    finally:
        for _, srcs, dsts in calls:
            for p in srcs[:2] + dsts:
                p.free()
        d.close()
