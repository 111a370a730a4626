"""``SMALFitter.fit_step`` as a captured hipGraph (``torch.cuda.CUDAGraph``): ~40 kernel launches replayed with a single call.
One rank: one graph.  Several ranks: ``[losses + backward] | all-reduce of the shared block | [Adam of every parameter]`` - two
graphs with the collective between them; the temporal-halo rows are received straight into two persistent device buffers the
first graph reads (posted before the replay, waited for in front of it: a graph cannot wait in its middle - the eager
``fit_step`` can, and does).  Worth it when the iteration is launch-bound (few frames); results are identical to the eager step."""
import torch

from . import engine
from .fit_epoch import addressed, cameras_part, params_part, raster_part, weights_part


def graph_key(f, weights, w_temp, window):
    """Everything a captured iteration bakes in besides the parameter buffers: loss weights, which parameters train,
    the target tensors, the rasteriser settings, and the raw device addresses of the camera tables, the rotation masks and the
    rasteriser workspace.  A replay happens only while all of them are what they were at capture time."""
    ws = f.device_model._ws
    addresses = (cameras_part(f.renderer, addressed), addressed(f.fov.data), addressed(f._mask_table()), addressed(f.log_beta_scales.data),
                 addressed(f.betas_trans.data), addressed(f.betas.data), None if ws is None else ws.data_ptr())
    # (the target signature as uploaded: ``step`` and every evaluation bring it in line first)
    return (weights_part(weights), float(w_temp), window, params_part(f, False), f._cache.target_signature, addresses, raster_part(f.renderer))


def step(f, weights, w_temp, window, ranks=None, group=None, shared_grad_hook=None, host_staged=False):
    """One replayed iteration (captured first when nothing captured fits); ``ranks=(rank, world)``: the two-graph form.
    Returns objs (10,) in a buffer that the next replay overwrites."""
    c = f._cache
    window = f.config.WINDOW_SIZE if window is None else window
    f._refresh_targets(force=False)
    f._mask_table()  # in-place mask edits since the capture reach the buffer the graph reads (outside the graph)
    prefix = ()
    if ranks is not None:
        from . import optimize  # (local: optimize imports nothing from here)

        prefix = ("ranks",) + tuple(ranks)
        if c.halo_buf is None:
            n_row = f._pose.shape[1] * 3 + 3
            c.halo_buf = (torch.zeros(n_row, device=f.device), torch.zeros(n_row, device=f.device))
        first, last = f.boundary_rows()
        pending = optimize.post_halos(first, last, ranks[0], ranks[1], group, host_staged=host_staged, recv_prev=c.halo_buf[0], recv_next=c.halo_buf[1])
        for buf, row in zip(c.halo_buf, pending.wait()):  # (host-staged rehearsals arrive in fresh tensors)
            if row is not None and row.data_ptr() != buf.data_ptr():
                buf.copy_(row)
    g = c.graph
    if g is None or g["key"] != prefix + graph_key(f, weights, w_temp, window):
        g = capture(f, weights, w_temp, window, ranks, prefix)
    if g["t_mirror"] != c.adam_step:  # eager steps in between: bring the device counter back in line
        c.adam_t.fill_(c.adam_step)
    c.adam_step += 1
    g["t_mirror"] = c.adam_step
    # (the replay's rasteriser kernels run on THIS stream, not on the one the graph was captured on: order them behind the last
    # user of the device's shared workspace, and make the next user wait for them)
    f.device_model._claim_workspace()
    g["graph"].replay()
    if ranks is not None:
        handle = shared_grad_hook(g["shared_block"]) if shared_grad_hook is not None else None
        if handle is not None:
            handle.wait()
        g["graph_adam"].replay()
    c.invalidate("parameters")
    return g["objs"]


def capture(f, weights, w_temp, window, ranks=None, prefix=()):
    """Capture the iteration: one graph (single rank), or - ``ranks=(rank, world)`` - the losses + backward and the Adam update as
    two graphs, the first reading the persistent halo buffers."""
    c, dev = f._cache, f.device
    halo_kw = {}
    if ranks is not None:
        halo_kw = dict(halo_prev=c.halo_buf[0] if ranks[0] > 0 else None, halo_next=c.halo_buf[1] if ranks[0] + 1 < ranks[1] else None)
    if c.adam_t is None:
        c.adam_t = torch.zeros(1, dtype=torch.int32, device=dev)
    h = c.adam_hyper
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        # eager dry run (no parameter update): sizes the rasteriser workspace and tells which parameters get a gradient
        _, grads = f._loss_and_grads(None, weights, w_temp, window=window, **halo_kw)
        list(f._adam_items(grads, c.adam_step + 1))  # (creates the moments of parameters the next step is the first for)
    torch.cuda.current_stream(dev).wait_stream(side)
    c.adam_t.fill_(c.adam_step)
    torch.cuda.synchronize(dev)

    def adam_all(grads):
        for p, gr, st, lr in f._adam_items(grads, None):  # (the dry run created every state)
            engine.adam_step_dev(p, gr.contiguous(), st["m"], st["v"], lr, c.adam_t, st["t0"], h["betas"][0], h["betas"][1], h["eps"])

    graph = torch.cuda.CUDAGraph()
    graph_adam = shared_block = None
    with torch.cuda.graph(graph):
        c.adam_t.add_(1)
        objs, grads = f._loss_and_grads(None, weights, w_temp, window=window, **halo_kw)
        if ranks is None:
            adam_all(grads)
        else:
            shared_block = c.block.tensor  # summed over the ranks in place between the two graphs
    if ranks is not None:
        graph_adam = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph_adam, pool=graph.pool()):
            adam_all(grads)
    # keyed on the state AFTER the dry run, which may have (re)allocated the rasteriser workspace
    c.graph = dict(key=prefix + graph_key(f, weights, w_temp, window), graph=graph, objs=objs, t_mirror=c.adam_step, graph_adam=graph_adam,
                   shared_block=shared_block, grads=grads, ws=f.device_model._ws)  # (the kernels hold raw pointers into this workspace tensor)
    return c.graph
