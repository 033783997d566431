"""The frozen stage (stem + max-pool + layer1: frozen weights, no gradient w.r.t. the images) of one padded image shape as static buffers +
one captured graph, and the bookkeeping of its prefetch: which batch was announced, which stages are alive.  Both engines (engine.Trainer,
engine.InferenceEngine) run it through this module.

A stage writes only its own buffers: the graph reads `images` and writes `xs` (fp32) and `x16s` (the bf16 twin, training only).  The forward reads
`x` / `x16`, which `land` fills from the staging buffers -- so a stage that runs ahead never writes what a running forward reads.
No method here switches streams, records events or synchronises: everything is enqueued on the CURRENT stream, and which stream that is and what
it is ordered behind stays with the engines."""
import torch


def batch_token(obj):
    """Identity of a batch as the caller hands it over: the image tensor object itself ([B,3,H,W], or a NestedTensor's `.tensors`)
    and its version counter -- an announced batch is recognised when the very same, unmodified tensor comes back.  None: a list of
    images (padded into a fresh tensor on arrival) cannot be announced."""
    t = obj.tensors if hasattr(obj, "tensors") else obj
    if not torch.is_tensor(t) or t.dim() != 4 or not t.is_cuda:
        return None
    return (id(t), t._version, t.data_ptr())


class FrozenStage:
    """Buffers + graph of one padded image shape.  `x16` / `x16s` are None without twins (inference)."""

    def __init__(self, images, x, xs, x16=None, x16s=None, graph=None):
        self.images, self.x, self.xs, self.x16, self.x16s, self.graph = images, x, xs, x16, x16s, graph
        self.token = self.keep = None       # the announced batch's identity, and the batch itself (alive, so its id cannot be re-used)

    def run(self, images):
        """In line: the stage of `images`, now.  Whatever was announced is spent."""
        self.images.copy_(images)
        self.graph.replay()
        self.token = self.keep = None

    def announce(self, images, token):
        """The stage of the batch the NEXT call will bring (`token`: its batch_token)."""
        self.images.copy_(images, non_blocking=True)
        self.graph.replay()
        self.token, self.keep = token, images

    def claim(self, token):
        """Is the staged output the one of batch `token`?  The announcement is forgotten either way."""
        hit = token is not None and self.token == token
        self.token = self.keep = None
        return hit

    def land(self, twin=True):
        """Staging buffers -> the buffers the forward (x) and the backward (x16) read."""
        if twin and self.x16s is not None:
            self.x16.copy_(self.x16s)
        self.x.copy_(self.xs)


class FrozenStages:
    """Padded image shape -> FrozenStage, most recently asked for last.  `capture(shape)` builds a missing one; `sync` runs before a stage is
    dropped by `trim` (its graph may still be running)."""

    def __init__(self, capture, sync=None):
        self._capture, self._sync, self._stages = capture, sync or torch.cuda.synchronize, {}

    def for_shape(self, shape):
        shape = tuple(shape)
        st = self._stages.pop(shape, None)
        if st is None:
            st = self._capture(shape)
        self._stages[shape] = st
        return st

    def get(self, shape):
        return self._stages.get(tuple(shape))

    def trim(self, in_use, limit=2):
        """Stages that nothing in `in_use` is (a batch was announced and never arrived): keep the newest `limit`."""
        used = {id(s) for s in in_use}
        idle = [shape for shape, s in self._stages.items() if id(s) not in used]
        for shape in idle[:max(0, len(idle) - limit)]:
            self._sync()
            del self._stages[shape]

    def release(self, stage, in_use):
        """Drop `stage` unless something in `in_use` is that stage (the caller has synchronised)."""
        if stage is None or any(s is stage for s in in_use):
            return
        for shape in [k for k, s in self._stages.items() if s is stage]:
            del self._stages[shape]

    def clear(self):
        self._stages.clear()

    def __len__(self):
        return len(self._stages)

    def __iter__(self):
        return iter(self._stages)

    def __contains__(self, shape):
        return tuple(shape) in self._stages


def capture_frozen_stage(body, shape, device, twins, mirror, stream, pool, capture_error_mode=None, before_warm=None):
    """Static buffers + the captured graph of `body.frozen_stage` for one padded image shape -> FrozenStage.  One warm run on `stream` (lazily
    cached tables exist before the capture), a device synchronisation, then the capture of the same call on `stream` into `pool`.
    `before_warm()` runs inside the scope, ahead of the warm run (the trainer rewrites the frozen layers' forward weight images there)."""
    from . import ops
    B, _, H, W = shape
    h, w = body.frozen_out_hw(H, W)
    out = (B, h, w, 256)
    images, x = torch.zeros(tuple(shape), device=device), torch.empty(out, device=device)
    x16, x16s = (torch.empty(out, device=device, dtype=torch.bfloat16) for _ in range(2)) if twins else (None, None)
    fs = FrozenStage(images, x, torch.empty(out, device=device), x16, x16s)
    # (a HIP CU-masked stream -- hipExtStreamCreateWithCUMask, leaving 16-64 CUs to the step's own latency-bound chain -- was tried:
    # with such a queue alive EVERY launch of the process slowed down, 9.3 -> 19 ms per step, in-line replays included:
    # profiles/r4_prefetch_ab_cumask.txt; an ordinary stream it is)
    with ops.scope(MIRROR=mirror, BRANCH_BESIDE=0):      # a LINEAR graph: every node runs on the stream it is launched on
        if before_warm is not None:
            before_warm()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            body.frozen_stage(fs.images, twins, out_to=(fs.xs, fs.x16s))
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        fs.graph = torch.cuda.CUDAGraph()
        mode = {"capture_error_mode": capture_error_mode} if capture_error_mode is not None else {}
        with torch.cuda.graph(fs.graph, pool=pool, stream=stream, **mode):
            body.frozen_stage(fs.images, twins, out_to=(fs.xs, fs.x16s))
    return fs
