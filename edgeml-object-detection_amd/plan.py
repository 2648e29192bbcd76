"""Static execution plans: the host side of the engine.

A detector forward for a fixed (batch, height, width) is, in the library (csrc/lower.hip), lowered
once into
  * a packed weight blob (BatchNorm folded in float64, conv weights K-contiguous
    [Cout][KH][KW][Cin] with K padded to 32 plus their bf16 planes, depthwise weights tap-major
    [K*K][C], SE fc weights transposed), uploaded once per model and shared by every plan of it;
  * one workspace (256-byte aligned carve-outs) holding every activation, the input staging buffer
    and the output buffers;
  * an array of edgedet_op records (numpy; struct = include/edgedet.h, the field layout of every
    kind = csrc/records.hpp) that libedgedet.so runs
    directly or captures into a hipGraph replayed per batch.
NativePlan is that plan on the Python side: the workspace as one torch allocation, the records
resolved against it, and the named buffers; ops.conv_record builds single records by hand for the
unit tests of the kernels, and Plan strings such records together for the executor's tests (no
lowering policy: no tile table, no switch).  The numpy pack helpers (fold_bn, pack_conv_weight, pack_dw_weight,
split_bf16x3) restate the library's packer independently, for the tests that check it.  Nothing here
computes detections: every FLOP runs in the HIP kernels of libedgedet.so.
"""
import ctypes
import os

import numpy as np
import torch

from . import ops

# Conv math of the compute-bound conv tiles: "bf16x6" (fp32 GEMM as six bf16 partial products on the
# bf16 matrix cores, error below one fp32 rounding per product; csrc/conv.hip) or "f32"
# (v_mfma_f32_32x32x2_f32).  Override with EDGEDET_CONV_MATH=f32.
CONV_MATH = os.environ.get("EDGEDET_CONV_MATH", "bf16x6")
if CONV_MATH not in ("bf16x6", "f32"):
    raise ValueError(f"EDGEDET_CONV_MATH must be 'bf16x6' or 'f32', got {CONV_MATH!r}")


def conv_key(op):
    """Shape key of a CONV op in the tuned tile table (data/conv_tiles_gfx950.json): what
    tools/tune_conv.py writes and the library's lowering looks up (csrc/lower.hip conv_key;
    tests/test_native_model.py holds the two to each other)."""
    i = op.i
    lin = int(i[7] == 1 and i[8] == 1 and i[9] == 1 and i[10] == 0)
    return ",".join(str(int(v)) for v in (i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], i[9], lin,
                                           int(op.p.get(6) is not None), int(op.p.get(7) is not None)))


def _bf16_rn(x):
    """float32 array -> (bf16 bit patterns as uint16, the bf16 values as float32), round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint32)
    return r.astype(np.uint16), (r << np.uint32(16)).view(np.float32)


def split_bf16x3(w):
    """fp32 packed weights w [Cout, Kpad] -> uint16 [3, Cout, Kpad]: x0 = RN(x), x1 = RN(x - x0),
    x2 = RN(x - x0 - x1) (= exact) of x = w, and of x = -w in the odd 32-wide K blocks (k // 32 odd):
    the weight operand of the bf16x6 conv tiles, whose sign-alternated stages subtract those blocks'
    sums (csrc/conv.hip conv_x6b_body; the same arithmetic as split_bf16x3_kernel)."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.shape[-1] % 32 == 0, "rows of Kpad, a multiple of 32"
    w = np.where((np.arange(w.shape[-1]) // 32) % 2 == 1, -w, w).astype(np.float32)
    h0, f0 = _bf16_rn(w)
    r1 = (w - f0).astype(np.float32)
    h1, f1 = _bf16_rn(r1)
    r2 = (r1 - f1).astype(np.float32)
    h2, _ = _bf16_rn(r2)
    return np.stack([h0, h1, h2])


# ------------------------------------------------------------------------------ weights
def fold_bn(w, gamma, beta, mean, var, eps):
    """Eval BatchNorm folded into the preceding bias-free conv (float64 math, float32 result)."""
    w = np.asarray(w, dtype=np.float64)
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    wf = w * scale.reshape((-1,) + (1,) * (w.ndim - 1))
    bf = np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * scale
    return wf.astype(np.float32), bf.astype(np.float32)


def pack_conv_weight(w_oihw, cin_pad=None):
    """[Cout][Cin][KH][KW] -> [Cout][Kpad] with K = KH*KW*Cin ordered (kh, kw, ci), zero padded."""
    w = np.asarray(w_oihw, dtype=np.float32)
    cout, cin, kh, kw = w.shape
    if cin_pad and cin_pad > cin:
        w = np.concatenate([w, np.zeros((cout, cin_pad - cin, kh, kw), np.float32)], axis=1)
        cin = cin_pad
    k = kh * kw * cin
    kpad = (k + 31) // 32 * 32
    out = np.zeros((cout, kpad), dtype=np.float32)
    out[:, :k] = w.transpose(0, 2, 3, 1).reshape(cout, k)
    return out, k, kpad, cin


def pack_dw_weight(w_c1kk):
    w = np.asarray(w_c1kk, dtype=np.float32)
    c, _, kh, kw = w.shape
    return w.reshape(c, kh * kw).T.copy()


# ------------------------------------------------------------------------------ arena + ops
_ESIZE = {}


def _esize(dtype):
    if dtype not in _ESIZE:
        _ESIZE[dtype] = torch.empty(0, dtype=dtype).element_size()
    return _ESIZE[dtype]


class Op:
    def __init__(self, kind, i=None, p=None, f=None, d=None, name="", lane=0):
        self.kind, self.name, self.lane = kind, name, lane
        self.i = dict(i or {})
        self.p = dict(p or {})
        self.f = dict(f or {})
        self.d = dict(d or {})


# ------------------------------------------------------------------------------ native plans
_DTYPES = {0: torch.float32, 1: torch.int32, 2: torch.int64, 3: torch.uint8, 4: torch.int16}


class NativeBuf:
    """A named carve-out of a NativePlan's workspace (edgedet_model_buffers)."""

    def __init__(self, plan, name, offset, nbytes, dtype, shape):
        # the workspace tensor, not the plan: no plan <-> buffer reference cycle, so a plan (its graph
        # and workspace) is released when its last user drops it, at a known point, never by a
        # garbage-collector pass on whatever thread triggers one (possibly while graphs are launching)
        self.arena, self.name, self.off, self.nbytes = plan.arena, name, int(offset), int(nbytes)
        self.dtype, self.shape = dtype, tuple(int(v) for v in shape)

    def ptr(self):
        return self.arena.data_ptr() + self.off

    def tensor(self):
        es = _esize(self.dtype)
        n = int(np.prod(self.shape))
        return self.arena[self.off:self.off + n * es].view(self.dtype).view(self.shape)


class Records:
    """An array of op records (`records`, with `graph` = None to start) that the library runs
    directly or captures into a hipGraph."""

    def run(self, stream=None):
        L = ops.lib()
        ops.check(L.edgedet_plan_run(self.records.ctypes.data_as(ctypes.c_void_p), len(self.records),
                                     ops.stream_handle(stream)))

    def capture(self, stream):
        """Capture the plan into a hipGraph on `stream` (a non-default torch.cuda.Stream)."""
        L = ops.lib()
        if self.graph is not None:
            L.edgedet_graph_destroy(self.graph)
            self.graph = None
        # warm the kernels' one-time attribute setup outside of capture
        with torch.cuda.stream(stream):
            self.run(stream)
        stream.synchronize()
        g = ctypes.c_void_p()
        ops.check(L.edgedet_graph_create(self.records.ctypes.data_as(ctypes.c_void_p), len(self.records),
                                         ops.stream_handle(stream), ctypes.byref(g)))
        self.graph = g
        # prime the instance (the library uploaded the graph; the first launches also settle the
        # runtime's per-graph state), so a timed or served batch never pays a first-launch cost
        for _ in range(2):
            self.replay(stream)
        stream.synchronize()
        return self

    def replay(self, stream):
        ops.check(ops.lib().edgedet_graph_launch(self.graph, ops.stream_handle(stream)))

    def __del__(self):
        try:
            if self.graph is not None and ops._LIB is not None:
                ops._LIB.edgedet_graph_destroy(self.graph)
        except Exception:
            pass


class NativePlan(Records):
    """The library's plan of (model, B, H, W, u8): workspace, resolved records, named buffers."""

    def __init__(self, model, B, H, W, u8, device):
        from . import native
        self.model, self.B, self.H, self.W, self.u8 = model, B, H, W, u8
        self.device = torch.device(device)
        kind, nc, rt = model.kind, model.num_classes, model.reduced_tail
        self.weights = model.weights(self.device)
        self.arena = torch.zeros(native.workspace_size(kind, B, H, W, nc, rt, u8), dtype=torch.uint8,
                                 device=self.device)
        L = ops.lib()
        if self.device.type == "cuda":
            ops.check(L.edgedet_model_prepare(native._kind(kind), nc, int(rt), B, H, W, int(u8),
                                              self.arena.data_ptr(), ops.stream_handle()))
        else:
            host = np.zeros(self.arena.numel(), np.uint8)
            ops.check(L.edgedet_model_prepare_host(native._kind(kind), nc, int(rt), B, H, W, int(u8),
                                                   host.ctypes.data, host.size))
            self.arena.copy_(torch.from_numpy(host))
        self.records = native.records(kind, B, H, W, self.weights.data_ptr(), self.arena.data_ptr(), nc, rt, u8)
        self.buffers = {}
        for b in native.buffers(kind, B, H, W, nc, rt, u8):
            name = bytes(b["name"]).split(b"\0", 1)[0].decode()
            self.buffers[name] = NativeBuf(self, name, b["offset"], b["nbytes"], _DTYPES[int(b["dtype"])],
                                           b["shape"][:int(b["ndim"])])
        names = native.op_names(kind, B, H, W, nc, rt, u8)
        by_ptr = {}
        for nb in self.buffers.values():
            by_ptr.setdefault(nb.ptr(), nb)
        self.ops = []
        for k, r in enumerate(self.records):
            op = Op(int(r["kind"]), {j: int(v) for j, v in enumerate(r["i"])},
                    {j: (by_ptr.get(int(v), int(v)) if v else None) for j, v in enumerate(r["p"])},
                    {j: float(v) for j, v in enumerate(r["f"])}, {j: float(v) for j, v in enumerate(r["d"])},
                    name=names[k], lane=int(r["i"][ops.LANE_FIELD]))
            self.ops.append(op)
        self.input = self.buffer("images")
        self.out_box, self.out_score = self.buffer("out.boxes"), self.buffer("out.scores")
        self.out_label, self.out_count = self.buffer("out.labels"), self.buffer("out.count")
        # (Ho, Wo, Hp, Wp) of the transform: its own record, or the SSD stem that folds it in
        pre = next((op for op in self.ops if op.kind == ops.PREPROCESS), None)
        if pre is not None:
            self.resized = tuple(int(pre.i[j]) for j in (3, 4, 5, 6))
        else:
            stem = next(op for op in self.ops if op.kind == ops.SSD_STEM)
            self.resized = (int(stem.i[1]), int(stem.i[2]), int(stem.i[1]), int(stem.i[2]))
        self.graph = None
        model.attach(self)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def buffer(self, name):
        try:
            return self.buffers[name]
        except KeyError:
            raise KeyError(f"plan has no buffer {name!r}") from None

    def finalize(self):
        return self

    @property
    def arena_bytes(self):
        return self.arena.numel()

    def summary(self):
        kinds = {}
        for op in self.ops:
            kinds[op.kind] = kinds.get(op.kind, 0) + 1
        return {"ops": len(self.ops), "by_kind": kinds, "arena_MB": self.arena_bytes / 2 ** 20,
                "weights_MB": self.weights.numel() / 2 ** 20}


# ------------------------------------------------------------------------------ hand-built plans
# Records put together by hand, for the executor's tests (tests/test_gpu_lanes.py: FORK / WAIT / JOIN
# around plain convs).  No lowering policy lives here: a conv gets the tile its caller names (0 = the
# kernel's own choice, csrc/conv.hip choose_tile), and nothing reads the tuned table or a switch.
class WeightPack:
    """Float32 arrays at 64-float boundaries of one device blob."""

    def __init__(self):
        self.arrays, self.size, self.device_blob = [], 0, None

    def add(self, arr):
        assert self.device_blob is None, "the pack is uploaded: its blob is fixed"
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        self.arrays.append((self.size, a))
        ref = WRef(self, self.size)
        self.size += (a.size + 63) // 64 * 64
        return ref

    def upload(self, device):
        host = np.zeros(self.size, dtype=np.float32)
        for off, a in self.arrays:
            host[off:off + a.size] = a
        self.device_blob = torch.from_numpy(host).to(device)


class WRef:
    def __init__(self, pack, off):
        self.pack, self.off = pack, off

    def ptr(self):
        return self.pack.device_blob.data_ptr() + 4 * self.off


class Buf:
    """A float32 activation of a hand-built plan: its own allocation."""

    def __init__(self, shape, device, name):
        self.name, self.data = name, torch.zeros(tuple(shape), dtype=torch.float32, device=device)

    def ptr(self):
        return self.data.data_ptr()

    def tensor(self):
        return self.data


class Plan(Records):
    """Records added one by one; `weights` is complete when the plan is made (uploaded here)."""

    def __init__(self, weights, device):
        self.weights, self.device, self.graph = weights, torch.device(device), None
        weights.upload(self.device)
        self.ops, self.bufs, self._recs, self._lane = [], [], [], 0

    def buf(self, shape, name=""):
        self.bufs.append(Buf(shape, self.device, name))
        return self.bufs[-1]

    def _append(self, rec, name):
        self._recs.append(rec)
        self.ops.append(Op(int(rec["kind"][0]), name=name, lane=int(rec["i"][0, ops.LANE_FIELD])))

    def add(self, rec, name=""):
        """One record, on the current lane."""
        rec["i"][0, ops.LANE_FIELD] = self._lane
        self._append(rec, name)

    def _sync(self, kind, name, *ints):
        """FORK / WAIT / JOIN: records of the caller's stream (lane 0) whatever the current lane."""
        rec = np.zeros(1, dtype=ops.OP_DTYPE)
        rec["kind"] = kind
        rec["i"][0, :len(ints)] = ints
        self._append(rec, name)

    def fork(self, nlanes):
        """Side lanes 1..nlanes start after everything issued so far (independent branches)."""
        self._forked = nlanes
        self._sync(ops.FORK, "fork", nlanes)

    def lane(self, k):
        """Issue the following records on lane k (0 = the caller's stream)."""
        self._lane = k

    def wait(self, lane, on):
        """Lane `lane` waits for everything issued so far on lane `on` (both forked, or 0)."""
        self._sync(ops.WAIT, f"wait{lane}<-{on}", lane, on)

    def join(self):
        self._lane = 0
        self._sync(ops.JOIN, "join", self._forked)

    def finalize(self):
        self.records = np.concatenate(self._recs)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return self


def conv_op(plan, x, x_shape, w, bias, cout, k, stride, pad, act, y, y_shape, K, Kpad, tile=0, name=""):
    """A plain CONV record (ops.conv_record) on the plan's current lane; x, y are Bufs, w, bias WRefs."""
    assert x.data.shape == tuple(x_shape) and y.data.shape == tuple(y_shape), name
    assert K == k * k * x_shape[3] and Kpad == (K + 31) // 32 * 32, (name, K, Kpad)
    plan.add(ops.conv_record(x_shape, cout, k, stride, pad, act, x.ptr(), w.ptr(), bias.ptr(), y.ptr(), tile=tile),
             name)
