"""Many tensors as one: where the tensors of a model go on the virtual axis of a one-launch kernel (place_on_axis), and
whether gradients lie back to back in one buffer (BackToBack).  The planned step (network/plan.py) leaves every parameter
gradient as a view of ONE flat f32 buffer with a fixed slot layout; data_parallel.DataParallel reduces that buffer as one
tensor and optim.Adam addresses the gradients relative to it."""
import torch

__all__ = ['BackToBack', 'LINE', 'place_on_axis']

LINE = 32               # 32-bit words of a 128-byte line


def place_on_axis(addrs, counts):
    """Where tensors at byte addresses `addrs` of `counts` 32-bit words go on a virtual word axis (csrc/multi_tensor.h),
    in the order given: each at the first free word that has the tensor's own phase in a 128-byte line, so that a chunk
    boundary of the axis is a line boundary of every large tensor.  Returns (first word of every tensor, end)."""
    offs = []
    v = 0
    for addr, n in zip(addrs, counts):
        v += (addr // 4 - v) % LINE
        offs.append(v)
        v += n
    return offs, v


class BackToBack:
    """`flat(grads)`: the gradients as ONE tensor if they are contiguous f32 views lying back to back (gaps of less than
    16 bytes: 16-byte slots) in one storage -- the planned step's flat buffer -- else None.  The full check (dtype,
    layout, storage, order) runs once; afterwards a step only compares the addresses with the layout found then (25 us
    for 161 gradients instead of 1 ms of Python on a host-bound step).

    `layout`: (byte offset of every gradient from the lowest one, index of the lowest, elements spanned) once they lay
    back to back -- a new tuple whenever the full check ran again -- else None."""

    def __init__(self):
        self.layout = None

    def flat(self, grads):
        g0 = grads[0]
        lay = self.layout
        if lay is not None and len(grads) == len(lay[0]):
            rel, lo_index, span = lay
            base = grads[lo_index].data_ptr()
            st = grads[lo_index].untyped_storage()
            if ([g.data_ptr() - base for g in grads] == rel and 0 <= base - st.data_ptr()
                    and base - st.data_ptr() + 4 * span <= st.nbytes()):
                return torch.empty(0, dtype=torch.float32, device=g0.device).set_(st, (base - st.data_ptr()) // 4, (span,))
        self.layout = None
        if any(g.dtype != torch.float32 or not g.is_contiguous() or g.device != g0.device for g in grads):
            return None
        st = g0.untyped_storage()
        if any(g.untyped_storage().data_ptr() != st.data_ptr() for g in grads):
            return None
        spans = sorted((g.storage_offset(), g.numel(), i) for i, g in enumerate(grads))
        for (a, n, _), (b, _, _) in zip(spans, spans[1:]):
            if not 0 <= b - (a + n) < 4:
                return None
        lo, hi = spans[0][0], spans[-1][0] + spans[-1][1]
        base = grads[spans[0][2]].data_ptr()
        self.layout = ([g.data_ptr() - base for g in grads], spans[0][2], hi - lo)
        return torch.empty(0, dtype=torch.float32, device=g0.device).set_(st, lo, (hi - lo,))
