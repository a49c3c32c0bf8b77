"""The next chunk's batch-local plan beside the streamed step at small batches
(PlanPipeline, B < 4,096): the overlapped schedule (plan of chunk c+1 on the
lowest-priority stream while k_stream trains chunk c) against the in-line one,
bit for bit; which schedule overlap=None takes; and the failsafe replay under
the overlapped schedule.

(k_stream's grid is unchanged by this schedule -- the launch still covers every
resident slot and its idle workgroups leave at once -- so there is no
variable-grid case here.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U1, I1 = 300, 120


def _zipf_stream(B, nb, seed):
    """Zipf items over 120 rows, uniform users over 300: rows recur inside a
    batch, in consecutive batches and across every chunk cut."""
    rng = np.random.default_rng(seed)
    n = B * nb
    u = rng.integers(0, U1, n).astype(np.int32)
    i = ((rng.zipf(1.3, n) - 1) % I1).astype(np.int32)
    j = ((rng.zipf(1.3, n) - 1) % I1).astype(np.int32)
    return u, i, j


def _tables(d, dev, seed=3):
    rng = np.random.default_rng(seed)
    P = (rng.standard_normal((U1, d)) * 0.2).astype(np.float32)
    Q = (rng.standard_normal((I1, d)) * 0.2).astype(np.float32)
    return [torch.tensor(P, device=dev), torch.tensor(Q, device=dev),
            torch.full((U1, d), 0.1, device=dev), torch.full((I1, d), 0.1, device=dev)]


def _run(ops, dev, B, d, chunk, trip, overlap, graph, stream=True, spin=None):
    pipe = ops.PlanPipeline(U1, I1, d, B, chunk, dev, overlap=overlap)
    pipe.set_stream(stream)
    if spin is not None:
        pipe.set_spin_limit(spin)
    tabs = _tables(d, dev)
    pipe.run(tabs, ops.StepHParams(adver=1, reg=0.01), *trip, graph=graph)
    pipe.resolve()
    torch.cuda.synchronize()
    # each context's last chunk: the last full one (ctx 0) and the short one (ctx 1)
    losses = [x for c in pipe.ctx for x in c.losses()]
    return pipe, tabs, losses


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("d", [8, 64])
@pytest.mark.parametrize("B", [512, 64])
def test_overlapped_equals_inline(ops, dev, B, d, graph):
    """17 batches in chunks of 5: three full chunks and a short one (the second
    context is re-planned at another size).  Tables, accumulators and both
    losses of the two schedules are the same bits; nothing gave up."""
    chunk, nb = 5, 17
    trip = tuple(torch.tensor(x, device=dev) for x in _zipf_stream(B, nb, seed=B + d))
    ref, want, want_l = _run(ops, dev, B, d, chunk, trip, False, graph)
    assert not ref.overlapped
    pipe, got, got_l = _run(ops, dev, B, d, chunk, trip, True, graph)
    assert pipe.overlapped
    assert pipe.step_errors() == 0 and pipe.stream_recoveries() == 0
    assert ref.step_errors() == 0 and ref.stream_recoveries() == 0
    for name, x, y in zip(("P", "Q", "accP", "accQ"), want, got):
        assert torch.equal(x, y), name
    for k, (x, y) in enumerate(zip(want_l, got_l)):
        assert torch.equal(x, y), f"losses[{k}]"


def test_default_choice(ops, dev):
    """overlap=None at B = 512: beside the step for a call of three chunks, in
    line for a call of one (read from the pipeline's state, not from timing)."""
    B, d, chunk = 512, 64, 4
    trip = tuple(torch.tensor(x, device=dev) for x in _zipf_stream(B, 3 * chunk, seed=11))
    pipe = ops.PlanPipeline(U1, I1, d, B, chunk, dev, overlap=None)
    tabs = _tables(d, dev)
    hp = ops.StepHParams(adver=1)
    pipe.run(tabs, hp, *trip)
    assert pipe.overlapped
    pipe.run(tabs, hp, *trip, first_batch=0, n_batches=chunk)
    assert not pipe.overlapped
    pipe.run(tabs, hp, *trip, first_batch=chunk, n_batches=2 * chunk)
    assert pipe.overlapped
    torch.cuda.synchronize()
    assert pipe.step_errors() == 0 and pipe.stream_recoveries() == 0
    # close() gives the plan stream back (twice is fine); a later run makes a new one
    pipe.close()
    pipe.close()
    assert pipe.side is None
    pipe.run(tabs, hp, *trip)
    assert pipe.overlapped and pipe.side is not None
    torch.cuda.synchronize()
    assert pipe.step_errors() == 0 and pipe.stream_recoveries() == 0
    pipe.close()
    off =ops.PlanPipeline(U1, I1, d, B, chunk, dev, overlap=False)
    off.run(_tables(d, dev), hp, *trip)
    assert not off.overlapped


def test_failsafe_replays_overlapped_chunks(ops, dev):
    """Spin limit 0 on a three-chunk overlapped pipeline: every streamed chunk
    gives up at its first unready poll (the library's bounded give-up), the first
    failure gates the later chunks of both contexts, and the re-plan of a context
    and the final settling replay them in order: three replays, the two-kernel
    schedule's bits, no step error."""
    B, d, chunk, nb = 512, 64, 4, 12
    trip = tuple(torch.tensor(x, device=dev) for x in _zipf_stream(B, nb, seed=17))
    _, want, want_l = _run(ops, dev, B, d, chunk, trip, False, True, stream=False)
    pipe, got, got_l = _run(ops, dev, B, d, chunk, trip, True, True, spin=0)
    assert pipe.overlapped
    assert pipe.stream_recoveries() == nb // chunk
    assert pipe.step_errors() == 0
    for name, x, y in zip(("P", "Q", "accP", "accQ"), want, got):
        assert torch.equal(x, y), name
    for k, (x, y) in enumerate(zip(want_l, got_l)):
        assert torch.equal(x, y), f"losses[{k}]"
