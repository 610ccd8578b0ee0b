"""ctypes binding of include/llamago.h — the host-side mirror of the reference's pkg/ml + pkg/llama API.

`MLLib(path)` wraps any shared library exporting that API.  The product instance comes from
`load_product()` (libllamago.so -> libllamahip.so -> MI355X) and raises if the HIP library is absent;
the test-suite wraps its CPU checker library with the same class.  Method names are the Go
names (ml.MulMat -> MLLib.MulMat, llama.Eval -> Model/Context.Eval).
"""
import ctypes as C
import os

import numpy as np

c_u32 = C.c_uint32
c_u64 = C.c_uint64
c_f32p = C.POINTER(C.c_float)
c_u32p = C.POINTER(c_u32)
VP = C.c_void_p


class HParams(C.Structure):
    """llama.HParams (llama.go:149-158)."""
    _fields_ = [(n, c_u32) for n in ("ctxSize", "vocabSize", "embdSize", "multSize", "headsCount", "layersCount", "rotCount", "f16")]


# dtype / op numeric values (ml.go:85-94, 133-174)
TYPE_F32, TYPE_F16, TYPE_I32 = 0, 1, 6
OP_NAMES = ["NONE", "DUP", "ADD", "SUB", "MUL", "DIV", "SQR", "SQRT", "SUM", "MEAN", "REPEAT", "ABS", "SGN", "NEG", "STEP",
            "RELU", "GELU", "SILU", "NORM", "RMS_NORM", "MUL_MAT", "SCALE", "CPY", "RESHAPE", "VIEW", "PERMUTE", "TRANSPOSE",
            "GET_ROWS", "DIAG_MASK_INF", "SOFT_MAX", "ROPE", "CONV_1D_1S", "CONV_1D_2S", "FLASH_ATTN", "FLASH_FF"]


class MLError(RuntimeError):
    pass


class MLLib:
    def __init__(self, path, mode=C.RTLD_LOCAL):
        if not os.path.exists(path):
            raise MLError(f"shared library not found: {path} (run `python -c 'import __graft_entry__ as g; g.build()'`)")
        self.path = path
        self.lib = L = C.CDLL(path, mode=mode)

        def sig(name, res, *args):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = list(args)
            return fn

        sig("ml_NewContext", VP, C.c_int, C.c_int, C.c_int)
        sig("ml_ReleaseContext", None, VP)
        sig("ml_LastError", C.c_char_p)
        sig("ml_NewTensor1D", VP, VP, C.c_int, c_u32)
        sig("ml_NewTensor2D", VP, VP, C.c_int, c_u32, c_u32)
        sig("ml_NewTensor3D", VP, VP, C.c_int, c_u32, c_u32, c_u32)
        sig("ml_NewFP32", VP, VP, C.c_float)
        sig("ml_TensorData", c_f32p, VP)
        sig("ml_TensorShape", None, VP, c_u32p, c_u32p)
        sig("ml_TensorOp", C.c_int, VP)
        sig("ml_Nelements", c_u64, VP)
        sig("ml_TensorRead", C.c_int, VP, VP, c_f32p, c_u64)
        sig("ml_TensorDirty", None, VP)
        sig("ml_FreeTensor", None, VP)
        for name in ("ml_Add", "ml_Mul", "ml_MulMat", "ml_Repeat", "ml_GetRows", "ml_Copy", "ml_Scale"):
            sig(name, VP, VP, VP, VP)
        for name in ("ml_RMSNorm", "ml_SoftMax", "ml_Silu"):
            sig(name, VP, VP, VP)
        sig("ml_View1D", VP, VP, VP, c_u32, c_u32)
        sig("ml_Permute", VP, VP, VP, c_u32, c_u32, c_u32, c_u32)
        sig("ml_Rope", VP, VP, VP, c_u32, c_u32, c_u32)
        sig("ml_Reshape3D", VP, VP, VP, c_u32, c_u32, c_u32)
        sig("ml_DiagMaskInf", VP, VP, VP, c_u32)
        sig("ml_NewGraph", VP)
        sig("ml_FreeGraph", None, VP)
        sig("ml_BuildForwardExpand", C.c_int, VP, VP)
        sig("ml_GraphNodesCount", c_u32, VP)
        sig("ml_GraphNode", VP, VP, c_u32)
        sig("ml_GraphCompute", C.c_int, VP, VP)
        sig("llama_LoadModel", VP, C.c_char_p, c_u32)
        sig("llama_NewSyntheticModel", VP, C.POINTER(HParams), c_u64, c_u32, c_u32)
        sig("llama_SaveModel", C.c_int, VP, C.c_char_p, C.c_int)
        sig("llama_FreeModel", None, VP)
        sig("llama_ModelHParams", None, VP, C.POINTER(HParams))
        sig("llama_ModelFFSize", c_u32, VP)
        sig("llama_ModelTensor", VP, VP, C.c_char_p)
        sig("llama_NewContext", VP, VP, c_u32, C.c_int, C.c_int, C.c_int)
        sig("llama_ReleaseContext", None, VP)
        sig("llama_Eval", C.c_int, VP, VP, c_u32p, c_u32, c_u32)
        sig("llama_Logits", c_f32p, VP)
        sig("llama_MLContext", VP, VP)
        sig("llama_GreedyDecode", C.c_int, VP, VP, c_u32p, c_u32, c_u32, c_u32p, c_f32p)
        sig("llama_SampleTopPTopK", C.c_int, VP, c_f32p, c_u32, c_u32p, c_u32, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u64, c_u32p)
        sig("llama_SampleDecode", C.c_int, VP, VP, c_u32p, c_u32, c_u32, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u32p)
        sig("llamago_SampleDebug", C.c_int, VP, c_f32p, c_u32, c_u32p, c_u32, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u64, c_u32p,
            c_u32p, c_f32p, c_u32p)

    # ---- helpers -------------------------------------------------------------------------------
    def last_error(self):
        return (self.lib.ml_LastError() or b"").decode()

    def _chk(self, handle, what):
        if not handle:
            raise MLError(f"{what}: {self.last_error()}")
        return handle

    # ---- llama.SampleTopPTopK (llama.go:455-707) ------------------------------------------------
    def SampleTopPTopK(self, ctx, logits, lastNTokens, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0, draw=0, debug=False):
        """One sampling call.  debug=True also returns (candidate ids, probabilities) in rank order after the topP rescale."""
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        ring = (c_u32 * max(1, len(lastNTokens)))(*[int(t) for t in lastNTokens])
        tok = c_u32(0)
        if not debug:
            rc = self.lib.llama_SampleTopPTopK(ctx, lg.ctypes.data_as(c_f32p), lg.size, ring, len(lastNTokens), topK, topP, temp, repeatPenalty, seed, draw,
                                               C.byref(tok))
            if rc:
                raise MLError(f"llama_SampleTopPTopK: {self.last_error()}")
            return tok.value
        ids = (c_u32 * topK)()
        probs = np.zeros(topK, dtype=np.float32)
        keep = c_u32(0)
        rc = self.lib.llamago_SampleDebug(ctx, lg.ctypes.data_as(c_f32p), lg.size, ring, len(lastNTokens), topK, topP, temp, repeatPenalty, seed, draw,
                                          C.byref(tok), ids, probs.ctypes.data_as(c_f32p), C.byref(keep))
        if rc:
            raise MLError(f"llama_SampleTopPTopK: {self.last_error()}")
        return tok.value, list(ids)[:keep.value], probs[:keep.value].copy()

    # ---- ml.* ------------------------------------------------------------------------------------
    def NewContext(self, maxThreads=1, useAVX=False, useNEON=False):
        return self._chk(self.lib.ml_NewContext(maxThreads, int(useAVX), int(useNEON)), "ml_NewContext")

    def ReleaseContext(self, ctx):
        self.lib.ml_ReleaseContext(ctx)

    def NewTensor(self, ctx, ne, dt=TYPE_F32, data=None):
        ne = tuple(int(x) for x in ne)
        if len(ne) == 1:
            t = self.lib.ml_NewTensor1D(ctx, dt, ne[0])
        elif len(ne) == 2:
            t = self.lib.ml_NewTensor2D(ctx, dt, ne[0], ne[1])
        elif len(ne) == 3:
            t = self.lib.ml_NewTensor3D(ctx, dt, ne[0], ne[1], ne[2])
        else:
            raise ValueError("1..3 dims")
        self._chk(t, "ml_NewTensor")
        if data is not None:
            self.set_data(t, data)
        return t

    def NewFP32(self, ctx, v):
        return self._chk(self.lib.ml_NewFP32(ctx, float(v)), "ml_NewFP32")

    def data(self, t):
        """Host view of Tensor.Data as a flat numpy array (no copy)."""
        n = self.lib.ml_Nelements(t)
        return np.ctypeslib.as_array(self.lib.ml_TensorData(t), shape=(n,))

    def set_data(self, t, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32).ravel()
        d = self.data(t)
        assert a.size == d.size, (a.size, d.size)
        d[:] = a
        self.lib.ml_TensorDirty(t)

    def shape(self, t):
        ne = (c_u32 * 4)()
        nb = (c_u32 * 4)()
        self.lib.ml_TensorShape(t, ne, nb)
        return tuple(ne), tuple(nb)

    def read(self, ctx, t):
        """Computed values of a (contiguous) tensor, shaped numpy-style [ne3,ne2,ne1,ne0] squeezed of leading 1s."""
        n = self.lib.ml_Nelements(t)
        out = np.empty(n, dtype=np.float32)
        if self.lib.ml_TensorRead(ctx, t, out.ctypes.data_as(c_f32p), n):
            raise MLError(f"ml_TensorRead: {self.last_error()}")
        ne, _ = self.shape(t)
        return out.reshape(ne[3], ne[2], ne[1], ne[0])

    def op2(self, name, ctx, a, b):
        return self._chk(getattr(self.lib, "ml_" + name)(ctx, a, b), "ml_" + name)

    def op1(self, name, ctx, a):
        return self._chk(getattr(self.lib, "ml_" + name)(ctx, a), "ml_" + name)

    def Add(self, ctx, a, b): return self.op2("Add", ctx, a, b)
    def Mul(self, ctx, a, b): return self.op2("Mul", ctx, a, b)
    def MulMat(self, ctx, a, b): return self.op2("MulMat", ctx, a, b)
    def Repeat(self, ctx, a, b): return self.op2("Repeat", ctx, a, b)
    def GetRows(self, ctx, a, b): return self.op2("GetRows", ctx, a, b)
    def Copy(self, ctx, a, b): return self.op2("Copy", ctx, a, b)
    def Scale(self, ctx, a, b): return self.op2("Scale", ctx, a, b)
    def RMSNorm(self, ctx, a): return self.op1("RMSNorm", ctx, a)
    def SoftMax(self, ctx, a): return self.op1("SoftMax", ctx, a)
    def Silu(self, ctx, a): return self.op1("Silu", ctx, a)
    def View1D(self, ctx, a, ne0, off): return self._chk(self.lib.ml_View1D(ctx, a, ne0, off), "ml_View1D")
    def Permute(self, ctx, a, a0, a1, a2, a3): return self._chk(self.lib.ml_Permute(ctx, a, a0, a1, a2, a3), "ml_Permute")
    def Rope(self, ctx, a, past, dims, mode): return self._chk(self.lib.ml_Rope(ctx, a, past, dims, mode), "ml_Rope")
    def Reshape3D(self, ctx, a, n0, n1, n2): return self._chk(self.lib.ml_Reshape3D(ctx, a, n0, n1, n2), "ml_Reshape3D")
    def DiagMaskInf(self, ctx, a, past): return self._chk(self.lib.ml_DiagMaskInf(ctx, a, past), "ml_DiagMaskInf")

    def NewGraph(self):
        return self._chk(self.lib.ml_NewGraph(), "ml_NewGraph")

    def FreeGraph(self, g):
        self.lib.ml_FreeGraph(g)

    def BuildForwardExpand(self, g, t):
        if self.lib.ml_BuildForwardExpand(g, t):
            raise MLError(f"ml_BuildForwardExpand: {self.last_error()}")

    def GraphCompute(self, ctx, g):
        if self.lib.ml_GraphCompute(ctx, g):
            raise MLError(f"ml_GraphCompute: {self.last_error()}")

    def graph_ops(self, g):
        return [OP_NAMES[self.lib.ml_TensorOp(self.lib.ml_GraphNode(g, i))] for i in range(self.lib.ml_GraphNodesCount(g))]

    # ---- llama.* -----------------------------------------------------------------------------------
    def NewSyntheticModel(self, hp, seed=1234, layer0=0, layer1=0):
        return Model(self, self._chk(self.lib.llama_NewSyntheticModel(C.byref(hp), seed, layer0, layer1), "llama_NewSyntheticModel"))

    def LoadModel(self, path, ctxSize):
        return Model(self, self._chk(self.lib.llama_LoadModel(os.fsencode(path), ctxSize), "llama_LoadModel"))

    def LoadModelKeepF16(self, path, ctxSize):
        """llamago_LoadModelKeepF16 (product only): LoadModel, except that a file whose weight matrices are all f16 keeps them f16 in HBM
        (Model.weight_type == 1); any other file loads as LoadModel loads it."""
        f = self.lib.llamago_LoadModelKeepF16
        f.restype, f.argtypes = VP, [C.c_char_p, C.c_uint32]
        return Model(self, self._chk(f(os.fsencode(path), ctxSize), "llamago_LoadModelKeepF16"))

    def LoadModelKeepQ4(self, path, ctxSize):
        """llamago_LoadModelKeepQ4 (product only): LoadModel, except that a file whose weight matrices are all Q4_0 keeps their blocks as they are in
        HBM (Model.weight_type == 2); any other file loads as LoadModel loads it."""
        f = self.lib.llamago_LoadModelKeepQ4
        f.restype, f.argtypes = VP, [C.c_char_p, C.c_uint32]
        return Model(self, self._chk(f(os.fsencode(path), ctxSize), "llamago_LoadModelKeepQ4"))


def make_hparams(vocab, embd, mult, heads, layers, ctx=128):
    hp = HParams()
    hp.ctxSize, hp.vocabSize, hp.embdSize, hp.multSize, hp.headsCount, hp.layersCount = ctx, vocab, embd, mult, heads, layers
    hp.rotCount, hp.f16 = embd // heads, 0
    return hp


# Named shapes (SURVEY §8 / BASELINE.json configs).  "tiny" is the unit-test twin.
SHAPES = {
    "tiny": dict(vocab=512, embd=256, mult=256, heads=4, layers=2),
    "small": dict(vocab=2048, embd=1024, mult=256, heads=8, layers=4),
    "7B": dict(vocab=32000, embd=4096, mult=256, heads=32, layers=32),
    "13B": dict(vocab=32000, embd=5120, mult=256, heads=40, layers=40),
    "65B": dict(vocab=32000, embd=8192, mult=256, heads=64, layers=80),
}
PROMPT = [1, 306, 4658, 278, 6593, 310, 2834, 338]  # fixed 8-token prompt


class Model:
    """llama.Model (llama.go:181-193)."""

    def __init__(self, ml, handle):
        self.ml, self.h = ml, handle
        self.hp = HParams()
        ml.lib.llama_ModelHParams(handle, C.byref(self.hp))
        self.ffSize = ml.lib.llama_ModelFFSize(handle)

    def tensor(self, name):
        return self.ml.lib.llama_ModelTensor(self.h, name.encode())

    def Save(self, path, ftype=0):
        if self.ml.lib.llama_SaveModel(self.h, os.fsencode(path), ftype):
            raise MLError("llama_SaveModel failed")

    def QuantizeQ8(self):
        """Block-int8 weight matrices (our format): product quantises in HBM; a checker library replaces
        its weights by the dequantised values."""
        f = self.ml.lib.llamago_QuantizeModelQ8
        f.restype, f.argtypes = C.c_int, [VP]
        if f(self.h):
            raise MLError(f"llamago_QuantizeModelQ8: {self.ml.last_error()}")
        return self

    def NarrowF16(self):
        """llamago_NarrowModelF16 (product only): every weight matrix converted to f16 in HBM (round to nearest even), the f32 copies released.
        Returns the number of elements whose value changed.  Before any context of the model exists."""
        f = self.ml.lib.llamago_NarrowModelF16
        f.restype, f.argtypes = C.c_int, [VP, C.POINTER(c_u64)]
        n = c_u64(0)
        if f(self.h, C.byref(n)):
            raise MLError(f"llamago_NarrowModelF16: {self.ml.last_error()}")
        return int(n.value)

    def WidenF16(self):
        """llamago_WidenModelF16 (product only): the inverse - an f32 model again, holding the narrowed values exactly."""
        f = self.ml.lib.llamago_WidenModelF16
        f.restype, f.argtypes = C.c_int, [VP]
        if f(self.h):
            raise MLError(f"llamago_WidenModelF16: {self.ml.last_error()}")
        return self

    def QuantizeQ4(self):
        """llamago_QuantizeModelQ4 (product only): every weight matrix quantised to block-int4 in HBM (20 bytes per 32 weights), the f32 copies
        released.  Before any context of the model exists."""
        f = self.ml.lib.llamago_QuantizeModelQ4
        f.restype, f.argtypes = C.c_int, [VP]
        if f(self.h):
            raise MLError(f"llamago_QuantizeModelQ4: {self.ml.last_error()}")
        return self

    def SaveQ4(self, path):
        """llamago_SaveModelQ4 (product only): a block-int4 model as a ggjt file of ftype 2 (LoadModelKeepQ4 reads it back block for block)."""
        f = self.ml.lib.llamago_SaveModelQ4
        f.restype, f.argtypes = C.c_int, [VP, C.c_char_p]
        if f(self.h, os.fsencode(path)):
            raise MLError(f"llamago_SaveModelQ4: {self.ml.last_error()}")

    def ExpandQ4(self):
        """llamago_ExpandModelQ4 (product only): a block-int4 model as the block-int8 model with the same quants and scales (identical values)."""
        f = self.ml.lib.llamago_ExpandModelQ4
        f.restype, f.argtypes = C.c_int, [VP]
        if f(self.h):
            raise MLError(f"llamago_ExpandModelQ4: {self.ml.last_error()}")
        return self

    @property
    def weight_type(self):
        """llamago_ModelWeightType (product only): 0 = f32, 1 = f16, 2 = block-int4, 7 = block-int8 weight matrices."""
        f = self.ml.lib.llamago_ModelWeightType
        f.restype, f.argtypes = C.c_int, [VP]
        return int(f(self.h))

    def SetTensor(self, name, values):
        """llamago_SetModelTensor (product only, test instrumentation): one fp32 tensor of the model overwritten in HBM; values in the layout read()
        shows (rows = ne1, columns = ne0).  Raises on an unknown name, a size mismatch, a quantised tensor or a model with live contexts."""
        f = self.ml.lib.llamago_SetModelTensor
        f.restype, f.argtypes = C.c_int, [VP, C.c_char_p, c_f32p, c_u64]
        a = np.ascontiguousarray(values, dtype=np.float32).ravel()
        if f(self.h, name.encode(), a.ctypes.data_as(c_f32p), a.size):
            raise MLError(f"llamago_SetModelTensor: {self.ml.last_error()}")
        return self

    def NewContext(self, ctxSize=128, maxThreads=1, useAVX=False, useNEON=False):
        h = self.ml._chk(self.ml.lib.llama_NewContext(self.h, ctxSize, maxThreads, int(useAVX), int(useNEON)), "llama_NewContext")
        return Context(self, h)

    def free(self):
        if self.h:
            self.ml.lib.llama_FreeModel(self.h)
            self.h = None


def _cache_read(ml, name, head, which, off, n):
    f = getattr(ml.lib, name)
    f.restype, f.argtypes = C.c_int, [VP] + [c_u32] * (len(head) - 1) + [C.c_int, c_u64, c_f32p, c_u64]
    out = np.empty(int(n), dtype=np.float32)
    if f(*head, int(which), int(off), out.ctypes.data_as(c_f32p), int(n)):
        raise MLError(f"{name}: {ml.last_error()}")
    return out


def _cache_write(ml, name, head, which, off, values):
    f = getattr(ml.lib, name)
    f.restype, f.argtypes = C.c_int, [VP] + [c_u32] * (len(head) - 1) + [C.c_int, c_u64, c_f32p, c_u64]
    a = np.ascontiguousarray(values, dtype=np.float32).ravel()
    if f(*head, int(which), int(off), a.ctypes.data_as(c_f32p), a.size):
        raise MLError(f"{name}: {ml.last_error()}")


class Context:
    """llama.Context (llama.go:83-88)."""

    def __init__(self, model, handle):
        self.model, self.ml, self.h = model, model.ml, handle

    def Eval(self, tokens, pastCount):
        toks = (c_u32 * len(tokens))(*[int(t) for t in tokens])
        if self.ml.lib.llama_Eval(self.h, self.model.h, toks, len(tokens), pastCount):
            raise MLError(f"llama_Eval: {self.ml.last_error()}")
        return self.logits()

    def logits(self):
        V = self.model.hp.vocabSize
        return np.ctypeslib.as_array(self.ml.lib.llama_Logits(self.h), shape=(V,)).copy()

    def GreedyDecode(self, prompt, n_predict, want_logits=True):
        V = self.model.hp.vocabSize
        toks = (c_u32 * len(prompt))(*[int(t) for t in prompt])
        out = (c_u32 * n_predict)()
        lg = np.empty((n_predict, V), dtype=np.float32) if want_logits else None
        rc = self.ml.lib.llama_GreedyDecode(self.h, self.model.h, toks, len(prompt), n_predict, out,
                                            lg.ctypes.data_as(c_f32p) if want_logits else None)
        if rc:
            raise MLError(f"llama_GreedyDecode: {self.ml.last_error()}")
        return list(out), lg

    def GreedyContinue(self, token, past, n_steps):
        """llamago_GreedyContinue: n_steps x { llama.Eval of one token through ml_GraphCompute, host argmax } from the context's present state."""
        L = self.ml.lib
        L.llamago_GreedyContinue.restype = C.c_int
        L.llamago_GreedyContinue.argtypes = [VP, VP, c_u32, c_u32, c_u32, c_u32p]
        out = (c_u32 * max(n_steps, 1))()
        if L.llamago_GreedyContinue(self.h, self.model.h, int(token), int(past), int(n_steps), out):
            raise MLError(f"llamago_GreedyContinue: {self.ml.last_error()}")
        return [int(t) for t in out[:n_steps]]

    def SetF16Stream(self, on=True):
        """llamago_SetF16Stream: Evals of an f16 model that take the stream kernels (2..128 rows) read the model's halves instead of a widened image."""
        L = self.ml.lib
        L.llamago_SetF16Stream.restype = C.c_int
        L.llamago_SetF16Stream.argtypes = [VP, C.c_int]
        if L.llamago_SetF16Stream(self.h, 1 if on else 0):
            raise MLError(f"llamago_SetF16Stream: {self.ml.last_error()}")

    @property
    def f16_stream(self):
        L = self.ml.lib
        L.llamago_F16Stream.restype = C.c_int
        L.llamago_F16Stream.argtypes = [VP]
        return bool(L.llamago_F16Stream(self.h))

    def SetQ4Stream(self, on=True):
        """llamago_SetQ4Stream: Evals of a block-int4 model over activation planes (5..88 rows) read the model's nibbles instead of an expanded int8 image."""
        L = self.ml.lib
        L.llamago_SetQ4Stream.restype = C.c_int
        L.llamago_SetQ4Stream.argtypes = [VP, C.c_int]
        if L.llamago_SetQ4Stream(self.h, 1 if on else 0):
            raise MLError(f"llamago_SetQ4Stream: {self.ml.last_error()}")

    @property
    def q4_stream(self):
        L = self.ml.lib
        L.llamago_Q4Stream.restype = C.c_int
        L.llamago_Q4Stream.argtypes = [VP]
        return bool(L.llamago_Q4Stream(self.h))

    def SetF16Tiles(self, on=True):
        """llamago_SetF16Tiles: Evals of an f16 model beyond 128 rows run their k_gemm_b9 launches on the model's halves (k_gemm_b9_h) instead of a widened image."""
        L = self.ml.lib
        L.llamago_SetF16Tiles.restype = C.c_int
        L.llamago_SetF16Tiles.argtypes = [VP, C.c_int]
        if L.llamago_SetF16Tiles(self.h, 1 if on else 0):
            raise MLError(f"llamago_SetF16Tiles: {self.ml.last_error()}")

    @property
    def f16_tiles(self):
        L = self.ml.lib
        L.llamago_F16Tiles.restype = C.c_int
        L.llamago_F16Tiles.argtypes = [VP]
        return bool(L.llamago_F16Tiles(self.h))

    def TimeComputes(self, on=True):
        """lh_ctx_time_computes: HIP events around every lh_graph_compute of this context; zeroes the sums."""
        L = self.ml.lib
        L.llamago_TimeComputes.restype = C.c_int
        L.llamago_TimeComputes.argtypes = [VP, C.c_int]
        if L.llamago_TimeComputes(self.h, 1 if on else 0):
            raise MLError(f"llamago_TimeComputes: {self.ml.last_error()}")

    def ComputeStats(self):
        """-> {"calls", "wall_us", "device_us"} summed over the lh_graph_compute calls since TimeComputes()."""
        L = self.ml.lib
        L.llamago_ComputeStats.restype = C.c_int
        L.llamago_ComputeStats.argtypes = [VP, C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        n, w, d = C.c_uint64(0), C.c_double(0), C.c_double(0)
        if L.llamago_ComputeStats(self.h, C.byref(n), C.byref(w), C.byref(d)):
            raise MLError("llamago_ComputeStats failed")
        return {"calls": int(n.value), "wall_us": float(w.value), "device_us": float(d.value)}

    def EnableEmbedding(self):
        """ModelParams.Embedding (llama.go:52): every Eval also leaves row N-1 of `embeddings` in lctx.Embedding (llama.go:414-419)."""
        self.ml.lib.llamago_EnableEmbedding.restype = None
        self.ml.lib.llamago_EnableEmbedding.argtypes = [VP]
        self.ml.lib.llamago_EnableEmbedding(self.h)

    def Embedding(self):
        self.ml.lib.llama_Embedding.restype = c_f32p
        self.ml.lib.llama_Embedding.argtypes = [VP]
        p = self.ml.lib.llama_Embedding(self.h)
        return np.ctypeslib.as_array(p, shape=(self.model.hp.embdSize,)).copy() if p else None

    def SetKeepCount(self, keep):
        """ModelParams.KeepCount (llama.go:47): what a context swap keeps (server.go:166-167)."""
        self.ml.lib.llamago_SetKeepCount.restype = None
        self.ml.lib.llamago_SetKeepCount.argtypes = [VP, c_u32]
        self.ml.lib.llamago_SetKeepCount(self.h, keep)

    def SampleDecode(self, prompt, n_predict, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0):
        """server.Do's generation loop (server.go:127-217) with SampleTopPTopK; returns the n_predict sampled ids."""
        toks = (c_u32 * len(prompt))(*[int(t) for t in prompt])
        out = (c_u32 * n_predict)()
        if self.ml.lib.llama_SampleDecode(self.h, self.model.h, toks, len(prompt), n_predict, topK, topP, temp, repeatPenalty, seed, out):
            raise MLError(f"llama_SampleDecode: {self.ml.last_error()}")
        return list(out)

    def Score(self, tokens, pastCount, targets=None):
        """llamago_Score: llama.Eval of `tokens` at pastCount with the lm_head for every row (llama.go:384), each row reduced on the device.
        Returns a structured array (ROW_SCORE_DTYPE) with one record per token; targets=None scores row i against tokens[i+1] and the
        last row against its own greedy id."""
        L = self.ml.lib
        L.llamago_Score.restype = C.c_int
        L.llamago_Score.argtypes = [VP, VP, c_u32p, c_u32, c_u32, c_u32p, C.POINTER(RowScore)]
        n = len(tokens)
        toks = (c_u32 * max(n, 1))(*[int(t) for t in tokens])
        tg = None
        if targets is not None:
            assert len(targets) == n, (len(targets), n)
            tg = (c_u32 * max(n, 1))(*[int(t) for t in targets])
        out = (RowScore * max(n, 1))()
        if L.llamago_Score(self.h, self.model.h, toks, n, int(pastCount), tg, out):
            raise MLError(f"llamago_Score: {self.ml.last_error()}")
        return np.frombuffer(out, dtype=ROW_SCORE_DTYPE, count=n).copy()

    def Verify(self, tokens, past, want_logits=False):
        """llamago_Verify: one verify pass of [pending token, draft...] on this context's cache at position `past` (lh_llama_verify).
        -> (ids of rows 0..a, a, logits of row a or None); the context then stands at past + a + 1."""
        L = self.ml.lib
        L.llamago_Verify.restype = C.c_int
        L.llamago_Verify.argtypes = [VP, c_u32p, c_u32, c_u32, c_u32p, c_u32p, c_f32p]
        n = len(tokens)
        toks = (c_u32 * max(n, 1))(*[int(t) for t in tokens])
        ids, a = (c_u32 * max(n, 1))(), c_u32(0)
        lg = np.empty(self.model.hp.vocabSize, dtype=np.float32) if want_logits else None
        if L.llamago_Verify(self.h, toks, n, int(past), ids, C.byref(a), lg.ctypes.data_as(c_f32p) if want_logits else None):
            raise MLError(f"llamago_Verify: {self.ml.last_error()}")
        return [int(t) for t in ids[:a.value + 1]], int(a.value), lg

    def DecodeLookup(self, first_token, past, n_steps, draft_max, ngram_max=3, ngram_min=1, corpus=None, want_logits=False):
        """llamago_DecodeLookup: the resident greedy loop through lookup-drafted verify passes (lh_llama_decode_lookup).
        -> (ids, last logits or None, stats dict(passes, rows, drafted, accepted, empty), trace list of (k, a) per pass)."""
        L = self.ml.lib
        L.llamago_DecodeLookup.restype = C.c_int
        L.llamago_DecodeLookup.argtypes = [VP, c_u32, c_u32, c_u32, C.POINTER(LookupParams), c_u32p, c_f32p, C.POINTER(SpecStats), C.POINTER(C.c_uint16), c_u32]
        lp, _keep = lookup_params(draft_max, ngram_max, ngram_min, corpus)
        n = max(int(n_steps), 1)
        out, st, tr = (c_u32 * n)(), SpecStats(), (C.c_uint16 * n)()
        lg = np.empty(self.model.hp.vocabSize, dtype=np.float32) if want_logits else None
        if L.llamago_DecodeLookup(self.h, int(first_token), int(past), int(n_steps), C.byref(lp), out, lg.ctypes.data_as(c_f32p) if want_logits else None,
                                  C.byref(st), tr, n):
            raise MLError(f"llamago_DecodeLookup: {self.ml.last_error()}")
        stats = dict(passes=int(st.passes), rows=int(st.rows), drafted=int(st.drafted), accepted=int(st.accepted), empty=int(st.empty))
        return [int(t) for t in out[:n_steps]], lg, stats, [(int(v) >> 8, int(v) & 0xFF) for v in tr[:min(st.passes, n)]]

    def SampleDecodeLookup(self, prompt, n_predict, draft_max, ngram_max=3, ngram_min=1, corpus=None, ring_size=0, topK=40, topP=0.95, temp=0.8,
                           repeatPenalty=1.10, seed=0):
        """llamago_SampleDecodeLookup: SampleDecode through lookup-drafted verify passes that sample every row (lh_llama_decode_sample_lookup);
        ring_size = 0: the reference's ring of ctxSize ids.  -> (the n_predict ids of SampleDecode, stats dict, trace list of (k, a) per pass)."""
        L = self.ml.lib
        L.llamago_SampleDecodeLookup.restype = C.c_int
        L.llamago_SampleDecodeLookup.argtypes = [VP, VP, c_u32p, c_u32, c_u32, c_u32, c_u32, C.c_float, C.c_float, C.c_float, c_u64, C.POINTER(LookupParams), c_u32p,
                                                 C.POINTER(SpecStats), C.POINTER(C.c_uint16), c_u32]
        lp, _keep = lookup_params(draft_max, ngram_max, ngram_min, corpus)
        toks = (c_u32 * max(len(prompt), 1))(*[int(t) for t in prompt])
        n = max(int(n_predict), 1)
        out, st, tr = (c_u32 * n)(), SpecStats(), (C.c_uint16 * n)()
        if L.llamago_SampleDecodeLookup(self.h, self.model.h, toks, len(prompt), int(n_predict), int(ring_size), int(topK), topP, temp, repeatPenalty, int(seed),
                                        C.byref(lp), out, C.byref(st), tr, n):
            raise MLError(f"llamago_SampleDecodeLookup: {self.ml.last_error()}")
        stats = dict(passes=int(st.passes), rows=int(st.rows), drafted=int(st.drafted), accepted=int(st.accepted), empty=int(st.empty))
        return [int(t) for t in out[:n_predict]], stats, [(int(v) >> 8, int(v) & 0xFF) for v in tr[:min(st.passes, n)]]

    def Perplexity(self, tokens, chunk=0):
        """llamago_Perplexity (convention: include/llamago_ext.h) -> (nll_sum, n_scored); perplexity = exp(nll_sum / n_scored)."""
        L = self.ml.lib
        L.llamago_Perplexity.restype = C.c_int
        L.llamago_Perplexity.argtypes = [VP, VP, c_u32p, c_u32, c_u32, C.POINTER(C.c_double), C.POINTER(c_u64)]
        toks = (c_u32 * max(len(tokens), 1))(*[int(t) for t in tokens])
        nll, cnt = C.c_double(0), c_u64(0)
        if L.llamago_Perplexity(self.h, self.model.h, toks, len(tokens), int(chunk), C.byref(nll), C.byref(cnt)):
            raise MLError(f"llamago_Perplexity: {self.ml.last_error()}")
        return float(nll.value), int(cnt.value)

    def CacheRead(self, which, off, n):
        """llamago_CacheRead (product only, test instrumentation): n floats at float offset `off` of the K (which = 0) or V (1) cache, behind everything
        the context's stream holds.  Layout [layer - layer0][position][channel]; raises on a range outside the cache."""
        return _cache_read(self.ml, "llamago_CacheRead", (self.h,), which, off, n)

    def CacheWrite(self, which, off, values):
        """llamago_CacheWrite (product only, test instrumentation): the floats `values` written at float offset `off` of the K / V cache."""
        _cache_write(self.ml, "llamago_CacheWrite", (self.h,), which, off, values)

    def PoisonWeightImages(self):
        """llamago_PoisonWeightImages (product only, test instrumentation): the fp32 / int8 images of f16 / block-int4 matrices on this context's lh_ctx
        filled with 0xFF bytes (NaN / quant -1) behind the work already enqueued -> the bytes filled (0: no such image exists)."""
        L = self.ml.lib
        L.llamago_PoisonWeightImages.restype = C.c_int64
        L.llamago_PoisonWeightImages.argtypes = [VP]
        n = L.llamago_PoisonWeightImages(self.h)
        if n < 0:
            raise MLError(f"llamago_PoisonWeightImages: {self.ml.last_error()}")
        return int(n)

    def free(self):
        if self.h:
            self.ml.lib.llama_ReleaseContext(self.h)
            self.h = None


LH_EINVAL, LH_EUNSUPPORTED = -1, -4   # include/llamahip.h


def _decode_draft(ml, fn, head, vocab, first_token, past, n_steps, draft_len, want_logits):
    """The shared body of llamago_DecodeDraft / llamago_DecodeDraftContexts (head = the pair, or the two contexts)."""
    fn.restype = C.c_int
    fn.argtypes = [VP] * len(head) + [c_u32, c_u32, c_u32, c_u32, c_u32p, c_f32p, C.POINTER(SpecStats), C.POINTER(C.c_uint16), c_u32]
    n = max(int(n_steps), 1)
    out, st, tr = (c_u32 * n)(), SpecStats(), (C.c_uint16 * n)()
    lg = np.empty(vocab, dtype=np.float32) if want_logits else None
    rc = fn(*head, int(first_token), int(past), int(n_steps), int(draft_len), out, lg.ctypes.data_as(c_f32p) if want_logits else None, C.byref(st), tr, n)
    if rc:
        e = MLError(f"llamago_DecodeDraft ({rc}): {ml.last_error()}")
        e.code = rc
        raise e
    stats = dict(passes=int(st.passes), rows=int(st.rows), drafted=int(st.drafted), accepted=int(st.accepted), empty=int(st.empty))
    return [int(t) for t in out[:n_steps]], lg, stats, [(int(v) >> 8, int(v) & 0xFF) for v in tr[:min(st.passes, n)]]


def decode_draft_contexts(target, draft, first_token, past, n_steps, draft_len, want_logits=False):
    """llamago_DecodeDraftContexts: the target's resident greedy loop through verify passes drafted by a second model's context (lh_llama_decode_draft; the
    rule is stated in include/llamahip.h and restated in tests/draft_model_ref.py).  The contexts of a DraftPair share a stream; any other two are refused.
    -> (ids, last logits or None, stats dict(passes, rows, drafted, accepted, empty), trace list of (k, a) per pass).  A refusal raises MLError whose
    `code` is the LH_E* code."""
    L = target.ml.lib
    return _decode_draft(target.ml, L.llamago_DecodeDraftContexts, (target.h, draft.h), target.model.hp.vocabSize, first_token, past, n_steps, draft_len, want_logits)


class _PairContext(Context):
    """A context that belongs to a DraftPair: llamago_FreeDraftPair releases it."""

    def free(self):
        self.h = None


class DraftPair:
    """llamago_NewDraftPair: a target and a draft context (one KV cache each) on ONE stream, for draft-model speculative decoding.  .target and .draft are
    ordinary Contexts (Eval, GreedyDecode, DecodeLookup, ...) that belong to the pair: free the pair, not them.  Evaluate the prompt on BOTH, then
    DecodeDraft."""

    def __init__(self, target_model, draft_model, ctx):
        self.ml = target_model.ml
        L = self.ml.lib
        L.llamago_NewDraftPair.restype, L.llamago_NewDraftPair.argtypes = VP, [VP, VP, c_u32]
        L.llamago_DraftPairTarget.restype, L.llamago_DraftPairTarget.argtypes = VP, [VP]
        L.llamago_DraftPairDraft.restype, L.llamago_DraftPairDraft.argtypes = VP, [VP]
        L.llamago_DraftPairReplaceDraft.restype, L.llamago_DraftPairReplaceDraft.argtypes = C.c_int, [VP, VP]
        L.llamago_FreeDraftPair.restype, L.llamago_FreeDraftPair.argtypes = None, [VP]
        self.h = self.ml._chk(L.llamago_NewDraftPair(target_model.h, draft_model.h, int(ctx)), "llamago_NewDraftPair")
        self.target = _PairContext(target_model, L.llamago_DraftPairTarget(self.h))
        self.draft = _PairContext(draft_model, L.llamago_DraftPairDraft(self.h))

    def ReplaceDraft(self, draft_model):
        """llamago_DraftPairReplaceDraft: the draft context freed, a fresh one (an empty cache) over draft_model in its place; the target stays."""
        L = self.ml.lib
        if L.llamago_DraftPairReplaceDraft(self.h, draft_model.h):      # (on failure the pair keeps its draft, and so does this object)
            raise MLError(f"llamago_DraftPairReplaceDraft: {self.ml.last_error()}")
        self.draft.h = None
        self.draft = _PairContext(draft_model, L.llamago_DraftPairDraft(self.h))
        return self.draft

    def DecodeDraft(self, first_token, past, n_steps, draft_len, want_logits=False):
        """llamago_DecodeDraft -> (ids, last logits or None, stats dict, trace list of (k, a)): the shape of Context.DecodeLookup."""
        L = self.ml.lib
        return _decode_draft(self.ml, L.llamago_DecodeDraft, (self.h,), self.target.model.hp.vocabSize, first_token, past, n_steps, draft_len, want_logits)

    def free(self):
        if self.h:
            self.target.h = self.draft.h = None
            self.ml.lib.llamago_FreeDraftPair(self.h)
            self.h = None


def usable_threads():
    """Host threads a harness may use: affinity mask capped by the cgroup CPU quota (the GPU box shows 256 logical CPUs under a
    16-CPU quota; oversubscribing the checker's OpenMP loops there is catastrophic)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, 64))


class KernelTime(C.Structure):
    """lh_kernel_time (include/llamahip.h)."""
    _fields_ = [("name", C.c_char * 48), ("launches", c_u32), ("total_ms", C.c_float), ("bytes_per_launch", c_u64)]


class RowScore(C.Structure):
    """lh_row_score (include/llamahip.h)."""
    _fields_ = [("logprob", C.c_double), ("lse", C.c_double), ("target_logit", C.c_float), ("max_logit", C.c_float), ("argmax", c_u32),
                ("target_rank", c_u32)]


ROW_SCORE_DTYPE = np.dtype([("logprob", "<f8"), ("lse", "<f8"), ("target_logit", "<f4"), ("max_logit", "<f4"), ("argmax", "<u4"), ("target_rank", "<u4")])


class LookupParams(C.Structure):
    """lh_lookup_params (include/llamahip.h)."""
    _fields_ = [("draft_max", c_u32), ("ngram_max", c_u32), ("ngram_min", c_u32), ("corpus", c_u32p), ("n_corpus", c_u32)]


class SpecStats(C.Structure):
    """lh_spec_stats (include/llamahip.h)."""
    _fields_ = [("passes", c_u32), ("rows", c_u32), ("drafted", c_u32), ("accepted", c_u32), ("empty", c_u32)]


def lookup_params(draft_max, ngram_max=3, ngram_min=1, corpus=None):
    """-> (LookupParams, the ctypes array its corpus pointer names: keep it alive for the call)."""
    arr = (c_u32 * len(corpus))(*[int(t) for t in corpus]) if corpus is not None and len(corpus) else None
    lp = LookupParams(int(draft_max), int(ngram_max), int(ngram_min), C.cast(arr, c_u32p) if arr is not None else None, len(corpus) if arr is not None else 0)
    return lp, arr


def draft_lookup(ml, window, draft_max, ngram_max=3, ngram_min=1, corpus=None, limit=None):
    """llamago_DraftLookup: the n-gram drafter alone on the device (lh_draft_lookup) -> the draft ids."""
    ml.lib.llamago_DraftLookup.restype = C.c_int
    ml.lib.llamago_DraftLookup.argtypes = [c_u32p, c_u32, C.POINTER(LookupParams), c_u32, c_u32p, c_u32p]
    lp, _keep = lookup_params(draft_max, ngram_max, ngram_min, corpus)
    win = (c_u32 * max(len(window), 1))(*[int(t) for t in window])
    out, k = (c_u32 * 8)(), c_u32(0)
    if ml.lib.llamago_DraftLookup(win, len(window), C.byref(lp), int(draft_max if limit is None else limit), out, C.byref(k)):
        raise MLError(f"llamago_DraftLookup: {ml.last_error()}")
    return [int(t) for t in out[:k.value]]


def spec_accept_pods(ml, arg, tok, k, pos, produced, n_steps, ctx):
    """llamago_SpecAcceptPods: the accept step of one pass of pods x R rows alone on the device (lh_spec_accept_pods; k_spec_accept_pods).  arg / tok
    [pods][R] = the rows' greedy ids / the tokens they evaluated; k, pos, produced [pods] = the pods' state in front of the pass.
    -> (a [pods], pos [pods], produced [pods], pending [pods], the ids appended per pod)."""
    arg = np.ascontiguousarray(arg, dtype=np.uint32)
    tok = np.ascontiguousarray(tok, dtype=np.uint32)
    P, R = (arg.shape if arg.ndim == 2 else (0, 0))
    assert tok.shape == arg.shape and len(k) == len(pos) == len(produced) == P, (arg.shape, tok.shape, len(k), len(pos), len(produced))
    f = ml.lib.llamago_SpecAcceptPods
    f.restype = C.c_int
    f.argtypes = [c_u32p, c_u32p, c_u32, c_u32, c_u32p, c_u32p, c_u32p, c_u32, c_u32, c_u32p, c_u32p, c_u32p, c_u32p, c_u32p]
    m = max(P, 1)
    kk, pp, pr = ((c_u32 * m)(*[int(x) for x in v]) for v in (k, pos, produced))
    a, npos, nprod, pend = ((c_u32 * m)() for _ in range(4))
    ids = (c_u32 * max(P * R, 1))()
    if f(arg.ctypes.data_as(c_u32p), tok.ctypes.data_as(c_u32p), P, R, kk, pp, pr, int(n_steps), int(ctx), a, npos, nprod, pend, ids):
        raise MLError(f"llamago_SpecAcceptPods: {ml.last_error()}")
    appended = [[int(t) for t in ids[i * R:i * R + (nprod[i] - int(produced[i]))]] for i in range(P)]
    return [int(x) for x in a[:P]], [int(x) for x in npos[:P]], [int(x) for x in nprod[:P]], [int(x) for x in pend[:P]], appended


def score_rows(ml, logits, targets):
    """llamago_ScoreRows: every row of host logits [n_rows][V] scored against targets[row] on the device (lh_score_rows)."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim == 1:
        lg = lg[None, :]
    n, V = lg.shape
    assert len(targets) == n, (len(targets), n)
    ml.lib.llamago_ScoreRows.restype = C.c_int
    ml.lib.llamago_ScoreRows.argtypes = [c_f32p, c_u32, c_u32, c_u32p, C.POINTER(RowScore)]
    tg = (c_u32 * max(n, 1))(*[int(t) for t in targets])
    out = (RowScore * max(n, 1))()
    if ml.lib.llamago_ScoreRows(lg.ctypes.data_as(c_f32p), n, V, tg, out):
        raise MLError(f"llamago_ScoreRows: {ml.last_error()}")
    return np.frombuffer(out, dtype=ROW_SCORE_DTYPE, count=n).copy()


def argmax_rows(ml, logits, which):
    """llamago_ArgmaxRows: the greedy id of every row of host logits [n_rows][V] on the device (lh_argmax_rows); which = 0: k_argmax_advance
    once per row, which = 1: one k_batch_argmax launch over all rows.  -> uint32 array [n_rows]."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim == 1:
        lg = lg[None, :]
    n, V = lg.shape
    ml.lib.llamago_ArgmaxRows.restype = C.c_int
    ml.lib.llamago_ArgmaxRows.argtypes = [c_f32p, c_u32, c_u32, C.c_int, c_u32p]
    out = np.zeros(max(n, 1), dtype=np.uint32)
    if ml.lib.llamago_ArgmaxRows(lg.ctypes.data_as(c_f32p), n, V, int(which), out.ctypes.data_as(c_u32p)):
        raise MLError(f"llamago_ArgmaxRows: {ml.last_error()}")
    return out[:n]


def sample_rows(ml, logits, ring, ring_pos, tokens, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0, draw0=0):
    """llamago_SampleRows: the rows of a verify pass sampled in one launch (lh_sample_rows; k_sample_rows / k_sample_small_rows).  logits [n_rows][V];
    ring = the lastNTokens ring with ring_pos ids appended so far; tokens[0] = the pending token (ignored), tokens[1..] the draft.  Row r is sampling
    call draw0 + r over the ring as if tokens[1..r] had been appended.  -> uint32 array [n_rows]."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim == 1:
        lg = lg[None, :]
    n, V = lg.shape
    assert len(tokens) == n, (len(tokens), n)
    ml.lib.llamago_SampleRows.restype = C.c_int
    ml.lib.llamago_SampleRows.argtypes = [c_f32p, c_u32, c_u32, c_u32p, c_u32, c_u32, c_u32p, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u64, c_u32p]
    rg = (c_u32 * max(len(ring), 1))(*[int(t) for t in ring])
    tk = (c_u32 * max(n, 1))(*[int(t) for t in tokens])
    out = np.zeros(max(n, 8), dtype=np.uint32)
    if ml.lib.llamago_SampleRows(lg.ctypes.data_as(c_f32p), n, V, rg, len(ring), int(ring_pos), tk, int(topK), topP, temp, repeatPenalty, int(seed), int(draw0),
                                 out.ctypes.data_as(c_u32p)):
        raise MLError(f"llamago_SampleRows: {ml.last_error()}")
    return out[:n]


def SamplePods(ml, logits, rings, ring_pos, draws, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0):
    """llamago_SamplePods: the pods of a sampled tick in one launch (lh_sample_pods; k_sample_pods / k_sample_small_pods).  logits [n][V]; rings [n][ring_size]
    with ring_pos[i] ids appended so far; draws[i] = pod i's sampling call.  -> (ids [n], the rings behind the ids [n][ring_size], their ring_pos [n])."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    if lg.ndim == 1:
        lg = lg[None, :]
    n, V = lg.shape
    rg = np.ascontiguousarray(rings, dtype=np.uint32)
    rs = rg.size // n if n else 0
    rg = rg.reshape(n, rs)
    assert len(ring_pos) == n and len(draws) == n
    f = ml.lib.llamago_SamplePods
    f.restype = C.c_int
    f.argtypes = [c_f32p, c_u32, c_u32, c_u32p, c_u32, c_u32p, C.POINTER(c_u64), c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u32p, c_u32p, c_u32p]
    rp = (c_u32 * max(n, 1))(*[int(x) for x in ring_pos])
    dr = (c_u64 * max(n, 1))(*[int(x) for x in draws])
    out = np.zeros(max(n, 64), dtype=np.uint32)
    rout = np.zeros((max(n, 1), max(rs, 1)), dtype=np.uint32)
    pout = np.zeros(max(n, 64), dtype=np.uint32)
    if f(lg.ctypes.data_as(c_f32p), n, V, rg.ctypes.data_as(c_u32p), rs, rp, dr, int(topK), topP, temp, repeatPenalty, int(seed), out.ctypes.data_as(c_u32p),
         rout.ctypes.data_as(c_u32p), pout.ctypes.data_as(c_u32p)):
        raise MLError(f"llamago_SamplePods: {ml.last_error()}")
    return out[:n], rout[:n, :rs], pout[:n]


def sample_pod_rows(ml, logits, rings, ring_pos, draws, tokens, n_draft, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0):
    """llamago_SamplePodRows: the pods x R rows of a batch's verify pass sampled in one launch (lh_sample_pod_rows; k_sample_pod_rows /
    k_sample_small_pod_rows).  logits [P * R][V]; rings [P][ring_size] with ring_pos[i] ids appended so far; draws[i] = pod i's next sampling call; tokens
    [P][R] = per pod the pending token (ignored) and the draft; n_draft[i] = pod i's draft length.  Row r of pod i is sampling call draws[i] + r over ring i
    as if tokens[i][1..r] had been appended.  -> uint32 array [P][R], 0xFFFFFFFF in the rows behind a pod's draft."""
    tk = np.ascontiguousarray(tokens, dtype=np.uint32)
    P, R = (tk.shape if tk.ndim == 2 else (0, 0))
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    V = lg.shape[-1] if lg.ndim >= 1 and lg.size else 0
    rg = np.ascontiguousarray(rings, dtype=np.uint32)
    rs = rg.size // P if P else 0
    assert lg.size == P * R * V and len(ring_pos) == len(draws) == len(n_draft) == P, (lg.shape, tk.shape)
    f = ml.lib.llamago_SamplePodRows
    f.restype = C.c_int
    f.argtypes = [c_f32p, c_u32, c_u32, c_u32, c_u32p, c_u32, c_u32p, C.POINTER(c_u64), c_u32p, c_u32p, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u32p]
    m = max(P, 1)
    rp, nd = ((c_u32 * m)(*[int(x) for x in v]) for v in (ring_pos, n_draft))
    dr = (c_u64 * m)(*[int(x) for x in draws])
    out = np.full(max(P * R, 64), 0xFFFFFFFF, dtype=np.uint32)
    if f(lg.ctypes.data_as(c_f32p), P, R, V, rg.ctypes.data_as(c_u32p), rs, rp, dr, tk.ctypes.data_as(c_u32p), nd, int(topK), topP, temp, repeatPenalty, int(seed),
         out.ctypes.data_as(c_u32p)):
        raise MLError(f"llamago_SamplePodRows: {ml.last_error()}")
    return out[:P * R].reshape(P, R)


def spec_accept_sample_pods(ml, arg, tok, k, pos, produced, n_steps, ctx, rings, ring_pos, draws):
    """llamago_SpecAcceptSamplePods: spec_accept_pods with the sampled commit (lh_spec_accept_sample_pods; k_spec_accept_pods on the sampled route).  rings
    [pods][ring_size], ring_pos / draws [pods] = the pods' sampler state in front of the pass.
    -> (a, pos, produced, pending, the ids appended per pod, rings [pods][ring_size], ring_pos [pods], draws [pods])."""
    arg = np.ascontiguousarray(arg, dtype=np.uint32)
    tok = np.ascontiguousarray(tok, dtype=np.uint32)
    P, R = (arg.shape if arg.ndim == 2 else (0, 0))
    rg = np.ascontiguousarray(rings, dtype=np.uint32)
    rs = rg.size // P if P else 0
    assert tok.shape == arg.shape and len(k) == len(pos) == len(produced) == len(ring_pos) == len(draws) == P
    f = ml.lib.llamago_SpecAcceptSamplePods
    f.restype = C.c_int
    f.argtypes = [c_u32p, c_u32p, c_u32, c_u32, c_u32p, c_u32p, c_u32p, c_u32, c_u32, c_u32p, c_u32, c_u32p, C.POINTER(c_u64), c_u32p, c_u32p, c_u32p, c_u32p, c_u32p,
                  c_u32p, c_u32p, C.POINTER(c_u64)]
    m = max(P, 1)
    kk, pp, pr, rp = ((c_u32 * m)(*[int(x) for x in v]) for v in (k, pos, produced, ring_pos))
    dr = (c_u64 * m)(*[int(x) for x in draws])
    a, npos, nprod, pend, rpo = ((c_u32 * m)() for _ in range(5))
    dro = (c_u64 * m)()
    ids = (c_u32 * max(P * R, 1))()
    rout = np.zeros((m, max(rs, 1)), dtype=np.uint32)
    if f(arg.ctypes.data_as(c_u32p), tok.ctypes.data_as(c_u32p), P, R, kk, pp, pr, int(n_steps), int(ctx), rg.ctypes.data_as(c_u32p), rs, rp, dr, a, npos, nprod, pend,
         ids, rout.ctypes.data_as(c_u32p), rpo, dro):
        raise MLError(f"llamago_SpecAcceptSamplePods: {ml.last_error()}")
    appended = [[int(t) for t in ids[i * R:i * R + (nprod[i] - int(produced[i]))]] for i in range(P)]
    return ([int(x) for x in a[:P]], [int(x) for x in npos[:P]], [int(x) for x in nprod[:P]], [int(x) for x in pend[:P]], appended,
            rout.reshape(-1)[:P * rs].reshape(P, rs), [int(x) for x in rpo[:P]], [int(x) for x in dro[:P]])


FEED_NEW, FEED_PENDING = 1, 2   # include/llamahip.h: LH_FEED_NEW, LH_FEED_PENDING


def _bind_extensions(ml):
    """Product-only entry points (no counterpart in the reference): resident decode loop, kernel timing, pipeline stage."""
    L = ml.lib
    L.llamago_DecodeGreedyResident.restype = C.c_int
    L.llamago_DecodeGreedyResident.argtypes = [VP, c_u32, c_u32, c_u32, c_u32p, c_f32p]
    L.llamago_ProfileDecode.restype = C.c_int
    L.llamago_ProfileDecode.argtypes = [VP, c_u32, c_u32, c_u32, C.POINTER(KernelTime), c_u32]
    L.llamago_Stage.restype = C.c_int
    L.llamago_Stage.argtypes = [VP, c_u32p, VP, VP, VP, c_u32, c_u32, VP, VP]
    L.llamago_Sync.restype = C.c_int
    L.llamago_Sync.argtypes = [VP]
    L.llamago_SetStream.restype = None
    L.llamago_SetStream.argtypes = [VP]
    L.llamago_DeviceCount.restype = C.c_int
    L.llamago_HbmReadProbe.restype = C.c_int
    L.llamago_HbmReadProbe.argtypes = [c_u64, c_u32, c_f32p]
    L.llamago_LastGraphFused.restype = C.c_int
    L.llamago_LastGraphFused.argtypes = [VP]
    L.llamago_GraphComputeNoFusion.restype = C.c_int
    L.llamago_GraphComputeNoFusion.argtypes = [VP, VP]
    L.llamago_CommUniqueId.restype = C.c_int
    L.llamago_CommUniqueId.argtypes = [C.POINTER(C.c_uint8)]
    L.llamago_NewPipeline.restype = VP
    L.llamago_NewPipeline.argtypes = [VP, c_u32, c_u32, C.c_int, C.c_int, C.POINTER(C.c_uint8), VP]
    L.llamago_NewPipelineGrouped.restype = VP
    L.llamago_NewPipelineGrouped.argtypes = [VP, c_u32, c_u32, C.c_int, C.c_int, C.POINTER(C.c_uint8), VP, c_u32]
    L.llamago_PipelineGroups.restype = c_u32
    L.llamago_PipelineGroups.argtypes = [VP]
    L.llamago_PipelineRunSample.restype = C.c_int
    L.llamago_PipelineRunSample.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32, c_u32, C.c_float, C.c_float, C.c_float, c_u64, c_u32]
    L.llamago_NewBatch.restype = VP
    L.llamago_NewBatch.argtypes = [VP, c_u32, c_u32]
    L.llamago_FreeBatch.restype = None
    L.llamago_FreeBatch.argtypes = [VP]
    L.llamago_BatchBatched.restype = C.c_int
    L.llamago_BatchBatched.argtypes = [VP]
    L.llamago_BatchGreedyDecode.restype = C.c_int
    L.llamago_BatchGreedyDecode.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32, c_u32p, c_f32p]
    L.llamago_BatchPrompt.restype = C.c_int
    L.llamago_BatchPrompt.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32p]
    L.llamago_BatchTick.restype = C.c_int
    L.llamago_BatchTick.argtypes = [VP, c_u32p]
    L.llamago_BatchSet.restype = C.c_int
    L.llamago_BatchSet.argtypes = [VP, c_u32p, c_u32p]
    L.llamago_BatchFeed.restype = C.c_int
    L.llamago_BatchFeed.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32p, c_u32p, c_f32p, c_f32p]
    L.llamago_BatchFeedSample.restype = C.c_int
    L.llamago_BatchFeedSample.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32p, c_u32p, c_u32p, c_f32p, c_f32p]
    L.llamago_BatchDecode.restype = C.c_int
    L.llamago_BatchDecode.argtypes = [VP, c_u32p, c_u32p, c_u32, c_u32p, c_f32p]
    L.llamago_BatchFork.restype = C.c_int
    L.llamago_BatchFork.argtypes = [VP, c_u32, c_u32p, c_u32, c_u32]
    L.llamago_BatchShareInfo.restype = C.c_int
    L.llamago_BatchShareInfo.argtypes = [VP, c_u32p, c_u32p]
    L.llamago_ShareSchedule.restype = C.c_int
    L.llamago_ShareSchedule.argtypes = [c_u32p, c_u32p, c_u32, c_u32, c_u32, C.POINTER(ShareBlock), c_u32, c_u32p]
    L.llamago_FreePipeline.restype = None
    L.llamago_FreePipeline.argtypes = [VP]
    L.llamago_PipelineRun.restype = C.c_int
    L.llamago_PipelineRun.argtypes = [VP, C.POINTER(c_u32p), c_u32p, c_u32]
    L.llamago_PipelineTokens.restype = C.c_int
    L.llamago_PipelineTokens.argtypes = [VP, c_u32, c_u32p, c_u32]
    L.llamago_PipelineProfileDecode.restype = C.c_int
    L.llamago_PipelineProfileDecode.argtypes = [VP, c_u32, c_u32, c_u32, C.POINTER(KernelTime), c_u32]
    L.llamago_PipelineSync.restype = C.c_int
    L.llamago_PipelineSync.argtypes = [VP]
    ml.has_extensions = True


COMM_ID_BYTES = 128


class ShareBlock(C.Structure):
    """lh_share_block: rows row[0..n) of a tick share the first `chunks` 128-key chunks of their caches."""
    _fields_ = [("n", c_u32), ("chunks", c_u32), ("row", c_u32 * 8)]


SHARE_NO_BLOCK = 0xFFFFFFFF


def share_schedule(ml, group, length, qb, min_rows, cap=None, sizing=False):
    """llamago_ShareSchedule (lh_share_schedule; no GPU): the block table a tick derives from the sharing groups of a batch.  group / length per pod
    as Batch.ShareInfo returns them.  -> (count, blocks as (chunks, [rows]) tuples, row_block list); count is -1 on bad arguments (blocks and row_block
    are then whatever was there: nothing is written).  sizing: the call without a block array; cap: the capacity handed over (default 32)."""
    rows = len(group)
    g = (c_u32 * max(rows, 1))(*[int(x) for x in group])
    ln = (c_u32 * max(rows, 1))(*[int(x) for x in length])
    cap = 32 if cap is None else int(cap)
    blocks = (ShareBlock * max(cap, 1))()
    rb = (c_u32 * max(rows, 1))(*([0xDEADBEEF] * max(rows, 1)))
    n = ml.lib.llamago_ShareSchedule(g, ln, rows, int(qb), int(min_rows), None if sizing else blocks, cap, rb)
    got = [] if sizing or n < 0 else [(int(blocks[i].chunks), [int(blocks[i].row[k]) for k in range(blocks[i].n)]) for i in range(min(n, cap))]
    return int(n), got, [int(x) for x in rb[:rows]]


def comm_unique_id(ml):
    """lh_comm_unique_id on this process's device: 128 bytes rank 0 hands to every other rank (any channel)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    if ml.lib.llamago_CommUniqueId(buf):
        raise MLError(f"llamago_CommUniqueId: {ml.last_error()}")
    return bytes(buf)


class Pipeline:
    """Pods as pipeline streams over a layer-sharded model (server.go:84-106, 151): this rank's stages of `pods` independent
    greedy streams, scheduled below the C-ABI (lh_pipeline_run) with RCCL send/recv of the residual stream.
    comm_id: bytes from comm_unique_id (RCCL), or None with `hooks` (an lh_comm_hooks ctypes struct: host-staged
    transport), or both None for world == 1."""

    def __init__(self, model, ctxSize, pods, rank=0, world=1, comm_id=None, hooks=None, max_rows=0):
        """max_rows: streams one tick evaluates together in ONE pass over the rank's weights (0 = as many as fit, 1 = every stream
        on its own: one weight pass per stream and tick)."""
        self.model, self.ml, self.pods, self.rank, self.world, self.ctxSize = model, model.ml, pods, rank, world, ctxSize
        idbuf = (C.c_uint8 * COMM_ID_BYTES)(*comm_id) if comm_id is not None else None
        self._hooks = hooks  # keep the callbacks alive
        h = self.ml.lib.llamago_NewPipelineGrouped(model.h, ctxSize, pods, rank, world, idbuf, C.byref(hooks) if hooks is not None else None, max_rows)
        self.h = self.ml._chk(h, "llamago_NewPipeline")
        self.groups = int(self.ml.lib.llamago_PipelineGroups(self.h))

    def _prompt_args(self, prompts):
        assert len(prompts) == self.pods
        arrs = [(c_u32 * len(p))(*[int(t) for t in p]) for p in prompts]
        pp = (c_u32p * self.pods)(*[C.cast(a, c_u32p) for a in arrs])
        nn = (c_u32 * self.pods)(*[len(p) for p in prompts])
        return arrs, pp, nn

    def run_sample(self, prompts=None, steps=0, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0, ringSize=0):
        """Like run(), with SampleTopPTopK on the last rank after every Eval (server.go:201-204); prompts on EVERY rank."""
        ring = ringSize or self.ctxSize
        if prompts is not None:
            keep, pp, nn = self._prompt_args(prompts)
            rc = self.ml.lib.llamago_PipelineRunSample(self.h, pp, nn, steps, topK, topP, temp, repeatPenalty, seed, ring)
        else:
            rc = self.ml.lib.llamago_PipelineRunSample(self.h, None, None, steps, topK, topP, temp, repeatPenalty, seed, ring)
        if rc:
            raise MLError(f"llamago_PipelineRunSample: {self.ml.last_error()}")

    def run(self, prompts=None, steps=0):
        """prompts: list of per-stream token lists (every rank passes them: the lengths shape the messages) or None to continue."""
        if prompts is not None:
            assert len(prompts) == self.pods
            arrs = [(c_u32 * len(p))(*[int(t) for t in p]) for p in prompts]
            pp = (c_u32p * self.pods)(*[C.cast(a, c_u32p) for a in arrs])
            nn = (c_u32 * self.pods)(*[len(p) for p in prompts])
            rc = self.ml.lib.llamago_PipelineRun(self.h, pp, nn, steps)
        else:
            rc = self.ml.lib.llamago_PipelineRun(self.h, None, None, steps)
        if rc:
            raise MLError(f"llamago_PipelineRun: {self.ml.last_error()}")

    def SetKeepCount(self, keep):
        """ModelParams.KeepCount of every stream (lh_pipeline_set_keep; the same value on every rank)."""
        self.ml.lib.llamago_PipelineSetKeepCount.argtypes = [VP, c_u32]
        if self.ml.lib.llamago_PipelineSetKeepCount(self.h, keep):
            raise MLError("llamago_PipelineSetKeepCount failed")

    def profile(self, on=True):
        """lh_pipeline_profile: HIP events around every stage and exchange of the following runs (clears the totals)."""
        self.ml.lib.llamago_PipelineProfile.argtypes = [VP, C.c_int]
        if self.ml.lib.llamago_PipelineProfile(self.h, 1 if on else 0):
            raise MLError("llamago_PipelineProfile failed")

    def stats(self):
        """Totals since profile(True): dict(ticks, stage_ms, exchange_ms) of THIS rank."""
        t, a, b = c_u32(0), C.c_float(0), C.c_float(0)
        self.ml.lib.llamago_PipelineStats.argtypes = [VP, c_u32p, c_f32p, c_f32p]
        if self.ml.lib.llamago_PipelineStats(self.h, C.byref(t), C.byref(a), C.byref(b)):
            raise MLError("llamago_PipelineStats failed")
        return dict(ticks=int(t.value), stage_ms=float(a.value), exchange_ms=float(b.value))

    def hop_probe(self, nbytes=16384, iters=1000):
        """Microseconds per ring shift of nbytes (every rank at the same time)."""
        us = C.c_float(0)
        self.ml.lib.llamago_PipelineHopProbe.argtypes = [VP, c_u32, c_u32, c_f32p]
        if self.ml.lib.llamago_PipelineHopProbe(self.h, nbytes, iters, C.byref(us)):
            raise MLError(f"llamago_PipelineHopProbe: {self.ml.last_error()}")
        return float(us.value)

    def tokens(self, pod):
        cap = 1 << 16
        out = (c_u32 * cap)()
        n = self.ml.lib.llamago_PipelineTokens(self.h, pod, out, cap)
        if n < 0:
            raise MLError(f"llamago_PipelineTokens: {self.ml.last_error()}")
        return list(out[:n])

    def profile_decode(self, token, past, repeats=2):
        arr = (KernelTime * 32)()
        n = self.ml.lib.llamago_PipelineProfileDecode(self.h, token, past, repeats, arr, 32)
        if n < 0:
            raise MLError(f"llamago_PipelineProfileDecode: {self.ml.last_error()}")
        return _kernel_times(arr, n)

    def free(self):
        if self.h:
            self.ml.lib.llamago_FreePipeline(self.h)
            self.h = None


class Batch:
    """`pods` llama.Contexts over one Model on ONE GPU whose decode steps share one pass over the weights (lh_batch; the reference
    runs its pods as independent goroutines, server.go:88-101)."""

    def __init__(self, model, ctxSize, pods):
        self.model, self.ml, self.pods = model, model.ml, pods
        self.h = self.ml._chk(self.ml.lib.llamago_NewBatch(model.h, ctxSize, pods), "llamago_NewBatch")
        self.batched = bool(self.ml.lib.llamago_BatchBatched(self.h))

    def SetQ4Stream(self, on=True):
        """llamago_BatchSetQ4Stream: Context.SetQ4Stream for the ticks, feeds and speculative passes of this batch."""
        L = self.ml.lib
        L.llamago_BatchSetQ4Stream.restype = C.c_int
        L.llamago_BatchSetQ4Stream.argtypes = [VP, C.c_int]
        if L.llamago_BatchSetQ4Stream(self.h, 1 if on else 0):
            raise MLError(f"llamago_BatchSetQ4Stream: {self.ml.last_error()}")

    @property
    def q4_stream(self):
        L = self.ml.lib
        L.llamago_BatchQ4Stream.restype = C.c_int
        L.llamago_BatchQ4Stream.argtypes = [VP]
        return bool(L.llamago_BatchQ4Stream(self.h))

    def SetF16Stream(self, on=True):
        """llamago_BatchSetF16Stream: Context.SetF16Stream for the ticks, feeds and speculative passes of this batch."""
        L = self.ml.lib
        L.llamago_BatchSetF16Stream.restype = C.c_int
        L.llamago_BatchSetF16Stream.argtypes = [VP, C.c_int]
        if L.llamago_BatchSetF16Stream(self.h, 1 if on else 0):
            raise MLError(f"llamago_BatchSetF16Stream: {self.ml.last_error()}")

    @property
    def f16_stream(self):
        L = self.ml.lib
        L.llamago_BatchF16Stream.restype = C.c_int
        L.llamago_BatchF16Stream.argtypes = [VP]
        return bool(L.llamago_BatchF16Stream(self.h))

    def GreedyDecode(self, prompts, n_predict, want_logits=False):
        """Every pod: its prompt as one Eval, then greedy steps; returns per pod the ids llama_GreedyDecode gives for its prompt alone."""
        assert len(prompts) == self.pods
        arrs = [(c_u32 * len(p))(*[int(t) for t in p]) for p in prompts]
        pp = (c_u32p * self.pods)(*[C.cast(a, c_u32p) for a in arrs])
        nn = (c_u32 * self.pods)(*[len(p) for p in prompts])
        out = (c_u32 * (self.pods * n_predict))()
        lg = np.empty((self.pods, self.model.hp.vocabSize), dtype=np.float32) if want_logits else None
        if self.ml.lib.llamago_BatchGreedyDecode(self.h, pp, nn, n_predict, out, lg.ctypes.data_as(c_f32p) if want_logits else None):
            raise MLError(f"llamago_BatchGreedyDecode: {self.ml.last_error()}")
        ids = [list(out[i * n_predict:(i + 1) * n_predict]) for i in range(self.pods)]
        return (ids, lg) if want_logits else ids

    def SetKeepCount(self, keep):
        self.ml.lib.llamago_BatchSetKeepCount.restype = None
        self.ml.lib.llamago_BatchSetKeepCount.argtypes = [VP, c_u32]
        self.ml.lib.llamago_BatchSetKeepCount(self.h, keep)

    def Prompt(self, prompts):
        """BatchHIP.Prompt (go/ml_hip_pods.go): every pod's prompt as one Eval; returns the id each prompt produced."""
        assert len(prompts) == self.pods
        arrs = [(c_u32 * len(p))(*[int(t) for t in p]) for p in prompts]
        pp = (c_u32p * self.pods)(*[C.cast(a, c_u32p) for a in arrs])
        nn = (c_u32 * self.pods)(*[len(p) for p in prompts])
        out = (c_u32 * self.pods)()
        if self.ml.lib.llamago_BatchPrompt(self.h, pp, nn, out):
            raise MLError(f"llamago_BatchPrompt: {self.ml.last_error()}")
        return list(out)

    def Set(self, tokens, past):
        """lh_batch_set: the token and the position of every pod's next tick, from the host (tokens None: the ids the device holds stay)."""
        tk = (c_u32 * self.pods)(*[int(t) for t in tokens]) if tokens is not None else None
        ps = (c_u32 * self.pods)(*[int(x) for x in past])
        if self.ml.lib.llamago_BatchSet(self.h, tk, ps):
            raise MLError(f"llamago_BatchSet: {self.ml.last_error()}")

    def _feed(self, name, tokens_per_pod, past, flags, want_logits, want_rows):
        """The marshalling of llamago_BatchFeed / llamago_BatchFeedSample (flags is None: the entry point takes none)."""
        assert len(tokens_per_pod) == self.pods and len(past) == self.pods
        arrs = [(c_u32 * max(len(p), 1))(*[int(t) for t in p]) for p in tokens_per_pod]
        pp = (c_u32p * self.pods)(*[C.cast(a, c_u32p) if len(p) else None for a, p in zip(arrs, tokens_per_pod)])
        nn = (c_u32 * self.pods)(*[len(p) for p in tokens_per_pod])
        ps = (c_u32 * self.pods)(*[int(x) for x in past])
        out = (c_u32 * self.pods)()
        V = self.model.hp.vocabSize
        last = np.full((self.pods, V), np.nan, dtype=np.float32) if want_logits else None
        rows = np.empty((sum(len(p) for p in tokens_per_pod), V), dtype=np.float32) if want_rows else None
        args = [self.h, pp, nn, ps] + ([] if flags is None else [flags[0]])
        args += [out, last.ctypes.data_as(c_f32p) if want_logits else None, rows.ctypes.data_as(c_f32p) if want_rows and rows.size else None]
        if getattr(self.ml.lib, name)(*args):
            raise MLError(f"{name}: {self.ml.last_error()}")
        res = ([int(out[i]) if len(p) else None for i, p in enumerate(tokens_per_pod)],)
        if want_logits:
            res += (last,)
        if want_rows:
            res += (rows,)
        return res if len(res) > 1 else res[0]

    def Feed(self, tokens_per_pod, past, want_logits=False, want_rows=False):
        """lh_batch_feed: llama.Eval of tokens_per_pod[i] at position past[i] of pod i's cache for every pod with a non-empty list, packed into
        shared weight passes; pods with an empty list are not fed.  Returns the list of ids (the greedy id of each fed pod's last row, None for
        pods that were not fed), then - if asked for - the [pods][vocab] logits of the fed pods' last rows (other rows NaN) and the
        [sum n][vocab] logits of every fed row, pods in index order."""
        return self._feed("llamago_BatchFeed", tokens_per_pod, past, None, want_logits, want_rows)

    def FeedSample(self, tokens_per_pod, past, flags=None, want_logits=False, want_rows=False):
        """lh_batch_feed_sample: Feed on a batch behind SetSampler.  flags[i]: FEED_NEW (pod i is a new job: ring and draw counter restart), FEED_PENDING
        (tokens[i][0] is the pod's pending id, in its ring already) or 0; None = all 0.  Returns as Feed, the ids being the ones sampled behind each fed
        pod's last row."""
        assert flags is None or len(flags) == self.pods
        fl = (c_u32 * self.pods)(*[int(x) for x in flags]) if flags is not None else None
        return self._feed("llamago_BatchFeedSample", tokens_per_pod, past, (fl,), want_logits, want_rows)

    def SetSampler(self, topK=40, topP=0.95, temp=0.8, repeatPenalty=1.10, seed=0, ringSize=64):
        """lh_batch_set_sampler: the following ticks sample (SampleTopPTopK on the device) instead of taking the argmax; allowed mid-stream."""
        f = self.ml.lib.llamago_BatchSetSampler
        f.restype, f.argtypes = C.c_int, [VP, c_u32, C.c_float, C.c_float, C.c_float, C.c_uint64, c_u32]
        if f(self.h, topK, topP, temp, repeatPenalty, seed, ringSize):
            raise MLError(f"llamago_BatchSetSampler: {self.ml.last_error()}")

    def ClearSampler(self):
        """lh_batch_set_sampler(NULL): back to greedy ticks."""
        f = self.ml.lib.llamago_BatchClearSampler
        f.restype, f.argtypes = C.c_int, [VP]
        if f(self.h):
            raise MLError(f"llamago_BatchClearSampler: {self.ml.last_error()}")

    def DecodeLookup(self, first_tokens, past, n_steps, draft_max, ngram_max=3, ngram_min=1, corpus=None, want_logits=False):
        """llamago_BatchDecodeLookup: n_steps greedy ids per pod from (first_tokens[i], past[i]) through lookup-drafted verify passes of pods x R rows
        (lh_batch_decode_lookup).  -> (ids per pod, [pods][vocab] logits behind each pod's last id or None, per pod a stats dict(passes, rows, drafted,
        accepted, empty), per pod the trace list of (k, a) per pass)."""
        return self._decode_lookup(self.ml.lib.llamago_BatchDecodeLookup, "llamago_BatchDecodeLookup", first_tokens, past, n_steps, draft_max, ngram_max, ngram_min,
                                   corpus, want_logits)

    def DecodeSampleLookup(self, first_tokens, past, n_steps, draft_max, ngram_max=3, ngram_min=1, corpus=None, want_logits=False):
        """llamago_BatchDecodeSampleLookup: DecodeLookup on a batch behind SetSampler (lh_batch_decode_sample_lookup) - the ids, rings and draw counters of
        Decode on the same batch, through verify passes whose pods x R rows are sampled in one launch.  Returns as DecodeLookup; the logits are the rows
        each pod's last id was sampled from."""
        return self._decode_lookup(self.ml.lib.llamago_BatchDecodeSampleLookup, "llamago_BatchDecodeSampleLookup", first_tokens, past, n_steps, draft_max, ngram_max,
                                   ngram_min, corpus, want_logits)

    def SamplerState(self, pod):
        """llamago_BatchSamplerRead (lh_batch_sampler_read): pod `pod`'s sampler state -> (ring as a list of ring_size ids, ring_pos, draw)."""
        f = self.ml.lib.llamago_BatchSamplerRead
        f.restype, f.argtypes = C.c_int, [VP, c_u32, c_u32p, c_u32p, C.POINTER(c_u64)]
        g = self.ml.lib.llamago_BatchSamplerRingSize
        g.restype, g.argtypes = c_u32, [VP]
        n = int(g(self.h))                     # 0: no sampler set - the read below says so
        ring, rp, dr = (c_u32 * max(n, 1))(), c_u32(0), c_u64(0)
        if f(self.h, int(pod), ring, C.byref(rp), C.byref(dr)):
            raise MLError(f"llamago_BatchSamplerRead: {self.ml.last_error()}")
        return [int(t) for t in ring[:n]], int(rp.value), int(dr.value)

    def _decode_lookup(self, fn, name, first_tokens, past, n_steps, draft_max, ngram_max, ngram_min, corpus, want_logits):
        assert len(first_tokens) == self.pods and len(past) == self.pods
        fn.restype = C.c_int
        fn.argtypes = [VP, c_u32p, c_u32p, c_u32, C.POINTER(LookupParams), c_u32p, c_f32p, C.POINTER(SpecStats), C.POINTER(C.c_uint16), c_u32]
        lp, _keep = lookup_params(draft_max, ngram_max, ngram_min, corpus)
        n = max(int(n_steps), 1)
        tk = (c_u32 * self.pods)(*[int(t) for t in first_tokens])
        ps = (c_u32 * self.pods)(*[int(x) for x in past])
        out, st, tr = (c_u32 * (self.pods * n))(), (SpecStats * self.pods)(), (C.c_uint16 * (self.pods * n))()
        lg = np.empty((self.pods, self.model.hp.vocabSize), dtype=np.float32) if want_logits else None
        if fn(self.h, tk, ps, int(n_steps), C.byref(lp), out, lg.ctypes.data_as(c_f32p) if want_logits else None, st, tr, n):
            raise MLError(f"{name}: {self.ml.last_error()}")
        ids = [[int(t) for t in out[i * n:i * n + n_steps]] for i in range(self.pods)]
        stats = [dict(passes=int(s.passes), rows=int(s.rows), drafted=int(s.drafted), accepted=int(s.accepted), empty=int(s.empty)) for s in st]
        traces = [[(int(v) >> 8, int(v) & 0xFF) for v in tr[i * n:i * n + min(st[i].passes, n)]] for i in range(self.pods)]
        return ids, lg, stats, traces

    def Decode(self, first_tokens, past, n_steps, want_logits=False):
        """lh_batch_decode: n_steps ticks of every pod from (first_tokens[i], past[i]).  -> ids per pod (and the [pods][vocab] logits of the last tick)."""
        assert len(first_tokens) == self.pods and len(past) == self.pods
        tk = (c_u32 * self.pods)(*[int(t) for t in first_tokens])
        ps = (c_u32 * self.pods)(*[int(x) for x in past])
        out = (c_u32 * (self.pods * n_steps))()
        lg = np.empty((self.pods, self.model.hp.vocabSize), dtype=np.float32) if want_logits else None
        if self.ml.lib.llamago_BatchDecode(self.h, tk, ps, int(n_steps), out, lg.ctypes.data_as(c_f32p) if want_logits else None):
            raise MLError(f"llamago_BatchDecode: {self.ml.last_error()}")
        ids = [[int(t) for t in out[i * n_steps:(i + 1) * n_steps]] for i in range(self.pods)]
        return (ids, lg) if want_logits else ids

    def Fork(self, src, dst, n_pos):
        """lh_batch_fork: cache rows [0, n_pos) and the token history of pod src copied into the pods of dst, which then share that prefix with src in
        the ticks (byte-equal results, the prefix's keys read once per block of member rows).  Feed each destination at past = n_pos, or Set it."""
        dst = [int(x) for x in dst]
        arr = (c_u32 * max(len(dst), 1))(*dst)
        if self.ml.lib.llamago_BatchFork(self.h, int(src), arr, len(dst), int(n_pos)):
            raise MLError(f"llamago_BatchFork: {self.ml.last_error()}")

    def ShareInfo(self):
        """lh_batch_share_info -> (group, length) per pod: the lowest pod index of the pod's sharing group and the shared length (own index, 0: none)."""
        g, ln = (c_u32 * self.pods)(), (c_u32 * self.pods)()
        if self.ml.lib.llamago_BatchShareInfo(self.h, g, ln):
            raise MLError(f"llamago_BatchShareInfo: {self.ml.last_error()}")
        return list(g), list(ln)

    def Tick(self):
        """BatchHIP.Tick: one decode step of every pod in one pass over the weights; returns the ids produced."""
        out = (c_u32 * self.pods)()
        if self.ml.lib.llamago_BatchTick(self.h, out):
            raise MLError(f"llamago_BatchTick: {self.ml.last_error()}")
        return list(out)

    def CacheRead(self, pod, which, off, n):
        """llamago_BatchCacheRead (test instrumentation): Context.CacheRead on pod `pod`'s cache."""
        return _cache_read(self.ml, "llamago_BatchCacheRead", (self.h, int(pod)), which, off, n)

    def CacheWrite(self, pod, which, off, values):
        """llamago_BatchCacheWrite (test instrumentation): Context.CacheWrite on pod `pod`'s cache."""
        _cache_write(self.ml, "llamago_BatchCacheWrite", (self.h, int(pod)), which, off, values)

    def PoisonWeightImages(self):
        """llamago_BatchPoisonWeightImages (test instrumentation): Context.PoisonWeightImages on the lh_ctx the batch evaluates in."""
        L = self.ml.lib
        L.llamago_BatchPoisonWeightImages.restype = C.c_int64
        L.llamago_BatchPoisonWeightImages.argtypes = [VP]
        n = L.llamago_BatchPoisonWeightImages(self.h)
        if n < 0:
            raise MLError(f"llamago_BatchPoisonWeightImages: {self.ml.last_error()}")
        return int(n)

    def free(self):
        if self.h:
            self.ml.lib.llamago_FreeBatch(self.h)
            self.h = None


def hbm_read_probe(ml, nbytes=4 << 30, repeats=4):
    """GB/s of a bare read-only HBM stream on this box (lh_hbm_read_probe)."""
    g = C.c_float(0)
    if ml.lib.llamago_HbmReadProbe(nbytes, repeats, C.byref(g)):
        raise MLError(f"llamago_HbmReadProbe: {ml.last_error()}")
    return float(g.value)


def decode_greedy_resident(ctx, first_token, past, n_steps, want_logits=False):
    """llamago_DecodeGreedyResident: n_steps decode steps without host round trips (argmax on the GPU)."""
    ml = ctx.ml
    out = (c_u32 * n_steps)()
    lg = np.empty(ctx.model.hp.vocabSize, dtype=np.float32) if want_logits else None
    if ml.lib.llamago_DecodeGreedyResident(ctx.h, first_token, past, n_steps, out, lg.ctypes.data_as(c_f32p) if want_logits else None):
        raise MLError(f"llamago_DecodeGreedyResident: {ml.last_error()}")
    return list(out), lg


def profile_decode(ctx, token, past, repeats=3):
    """Per-kernel-class HIP-event timing of eager decode steps: list of dicts(name, launches, avg_us, bytes_per_launch, gbps)."""
    ml = ctx.ml
    arr = (KernelTime * 32)()
    n = ml.lib.llamago_ProfileDecode(ctx.h, token, past, repeats, arr, 32)
    if n < 0:
        raise MLError(f"llamago_ProfileDecode: {ml.last_error()}")
    return _kernel_times(arr, n)


def _kernel_times(arr, n):
    res = []
    for i in range(n):
        k = arr[i]
        avg_us = k.total_ms * 1e3 / max(k.launches, 1)
        res.append(dict(name=k.name.decode(), launches=int(k.launches), avg_us=avg_us, bytes_per_launch=int(k.bytes_per_launch),
                        gbps=(k.bytes_per_launch / avg_us / 1e3) if avg_us > 0 else 0.0))
    return res


def route_trace(fn):
    """Run fn() with the calling thread's route trace on (include/llamahip.h lh_route_trace) and return (fn's result, the matmul instantiations
    it launched, in order).  Test instrumentation."""
    from . import LIBLLAMAHIP
    hip = C.CDLL(LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
    hip.lh_route_trace.restype = C.c_int
    hip.lh_route_trace.argtypes = [C.c_int]
    hip.lh_route_trace_read.restype = C.c_int64
    hip.lh_route_trace_read.argtypes = [C.c_char_p, C.c_uint64]
    hip.lh_route_trace(1)
    try:
        res = fn()
    finally:
        hip.lh_route_trace(0)
    buf = C.create_string_buffer(int(hip.lh_route_trace_read(None, 0)) + 16)
    hip.lh_route_trace_read(buf, len(buf))
    return res, buf.value.decode().split()


_product = None


def load_product():
    """The product library (HIP path).  Fails loudly when the extension is missing: there is no CPU fallback."""
    global _product
    if _product is None:
        from . import LIBLLAMAGO, LIBLLAMAHIP
        if not os.path.exists(LIBLLAMAHIP):
            raise MLError(f"HIP extension missing: {LIBLLAMAHIP} — build it with __graft_entry__.build(); no CPU fallback exists")
        hip = C.CDLL(LIBLLAMAHIP, mode=C.RTLD_GLOBAL)
        _product = MLLib(LIBLLAMAGO)
        _bind_extensions(_product)
        route_file = os.environ.get("LLAMAHIP_ROUTE_FILE")
        if route_file:   # test instrumentation (tests/test_gpu_zz_routes.py): this process appends the kernel families it launched when it exits
            import atexit
            hip.lh_route_log(1)
            hip.lh_route_names.restype = C.c_int64
            hip.lh_route_names.argtypes = [C.c_char_p, C.c_uint64]

            def _dump_routes():
                buf = C.create_string_buffer(int(hip.lh_route_names(None, 0)) + 16)
                hip.lh_route_names(buf, len(buf))
                with open(route_file, "a") as f:
                    f.write(buf.value.decode())
            atexit.register(_dump_routes)
    return _product
