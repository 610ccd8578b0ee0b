"""ctypes plumbing of the GPU tests that drive the node path through the raw C-ABI (include/llamahip.h) with graphs of tests/graph_ops_ref.py."""
import ctypes as C

import numpy as np

import graph_ops_ref as R

F32P = C.POINTER(C.c_float)
NO_FUSION = 1


def bind(lib):
    lib.lh_last_error.restype = C.c_char_p
    lib.lh_last_error.argtypes = [C.c_void_p]
    lib.lh_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.lh_ctx_destroy.argtypes = [C.c_void_p]
    lib.lh_tensor_register.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    lib.lh_graph_compute.argtypes = [C.c_void_p, C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.c_uint32]
    lib.lh_graph_check.argtypes = [C.POINTER(R.LhTensor), C.c_uint32, C.c_uint32, C.POINTER(R.LhBufExtent), C.c_uint32, C.c_char_p, C.c_uint64]
    lib.lh_node_read.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, F32P, C.c_uint64]
    lib.lh_buf_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, F32P, C.c_uint64]
    lib.lh_buf_free.argtypes = [C.c_void_p, C.c_uint64]
    lib.lh_route_trace.argtypes = [C.c_int]
    lib.lh_route_trace_read.restype = C.c_int64
    lib.lh_route_trace_read.argtypes = [C.c_char_p, C.c_uint64]
    return lib


class Session:
    """one lh_ctx; registered buffers are freed by close()"""

    def __init__(self, lib):
        self.lib, self.ctx, self.bufs = lib, C.c_void_p(), []
        assert lib.lh_ctx_create(0, None, C.byref(self.ctx)) == 0, lib.lh_last_error(None)

    def error(self):
        return (self.lib.lh_last_error(self.ctx) or b"").decode()

    def register(self, data):
        data = np.ascontiguousarray(data, dtype=np.float32)
        ne = (C.c_uint32 * 4)(data.size, 1, 1, 1)
        buf = C.c_uint64()
        assert self.lib.lh_tensor_register(self.ctx, 0, 0, ne, 0, data.ctypes.data, C.byref(buf)) == 0, self.error()
        self.bufs.append(buf.value)
        return buf.value

    def bound_graph(self, g, inputs):
        """a copy of g whose buffer ids are handles of freshly registered buffers holding `inputs`; {model id: handle}"""
        g = g.copy()
        handle = {bid: self.register(inputs[bid]) for bid in sorted(g.bufs)}
        g.bufs = {handle[bid]: v for bid, v in g.bufs.items()}
        for t in g.t:
            if t.buf:
                t.buf = handle[t.buf]
        return g, handle

    def check(self, g):
        arr, ext, nb = g.pack()
        msg = C.create_string_buffer(256)
        return self.lib.lh_graph_check(arr, *g.abi_counts(), ext, nb, msg, 256), msg.value.decode()

    def compute(self, g, flags):
        arr, _, _ = g.pack()
        return self.lib.lh_graph_compute(self.ctx, arr, *g.abi_counts(), flags)

    def read_buf(self, handle, n):
        out = np.empty(n, np.float32)
        assert self.lib.lh_buf_read(self.ctx, handle, 0, out.ctypes.data_as(F32P), n) == 0, self.error()
        return out

    def node_read(self, index, n, off=0):
        out = np.empty(n, np.float32)
        rc = self.lib.lh_node_read(self.ctx, index, off, out.ctypes.data_as(F32P), n)
        return rc, out

    def free_buffers(self):
        for b in self.bufs:
            self.lib.lh_buf_free(self.ctx, b)
        self.bufs = []

    def close(self):
        self.free_buffers()
        self.lib.lh_ctx_destroy(self.ctx)


def trace_of(lib, fn):
    """what the calling thread's matmul launch sites recorded while fn ran (include/llamahip.h lh_route_trace)"""
    lib.lh_route_trace(1)
    try:
        out = fn()
    finally:
        lib.lh_route_trace(0)
    buf = C.create_string_buffer(1 << 14)
    lib.lh_route_trace_read(buf, len(buf))
    return out, [ln for ln in buf.value.decode().split("\n") if ln]
