"""Host side of the train step, no GPU: every step global of conv / nn / segments / hrnet is switched by a scope of its owner that puts
back what it found; a failed forward pass leaves no BatchNorm counter behind; one abort rule; one bucket walk and one reduce body in
GradStore (expected values: the parent commit's GradStore on the same net)."""
import sys
import types

import pytest
import torch
import torch.nn as nn

from conftest import ROOT
sys.path.insert(0, ROOT)

from danet_densepose2smpl_amd import conv, hrnet, nn as dnn, segments, trainer      # noqa: E402
from danet_densepose2smpl_amd.distributed import GradStore                           # noqa: E402
from test_distributed import _Net                                                     # noqa: E402

BANK = conv.WeightBank()
STORE_A, STORE_B = object(), object()
# (scope, owner, attribute, a value the scope installs, another one, a non-default value to find on entry)
SCOPES = {
    'grad_store': (conv.grad_store, conv, 'GRAD_STORE', STORE_A, STORE_B, STORE_B),
    'deferred_wgrads': (conv.deferred_wgrads, conv, 'DEFER_WGRAD', True, False, True),
    'onepass_blocks': (dnn.onepass_blocks, dnn, 'ONEPASS_MAX_BLOCKS', 464, -1, 12),
    'segments': (segments.recording, segments, 'ACTIVE', True, False, True),
    'branch_streams': (hrnet.branch_streams, hrnet, 'BRANCH_STREAMS', True, False, True),
    'fresh_packs': (lambda v: conv.fresh_packs(), conv, 'RECORDER', None, None, BANK),
    'batch_counts': (lambda v: dnn.deferred_batch_counts(), dnn.BatchNorm2d, 'count_batches', False, False, False),
}


def _resting():
    """Every global a step switches, as (name, value) pairs."""
    return [('GRAD_STORE', conv.GRAD_STORE), ('DEFER_WGRAD', conv.DEFER_WGRAD), ('RECORDER', conv.RECORDER),
            ('ONEPASS_MAX_BLOCKS', dnn.ONEPASS_MAX_BLOCKS), ('SIDE_LIVE', dnn.SIDE_LIVE), ('count_batches', dnn.BatchNorm2d.count_batches),
            ('_ran', list(dnn.BatchNorm2d._ran)), ('ACTIVE', segments.ACTIVE), ('level', segments.level()),
            ('BRANCH_STREAMS', hrnet.BRANCH_STREAMS), ('queues', (len(conv._WQ), len(conv._WQG)))]


@pytest.mark.parametrize('found_default', [True, False], ids=['default_found', 'other_found'])
@pytest.mark.parametrize('name', sorted(SCOPES))
def test_scope_restores_what_it_found(name, found_default):
    scope, owner, attr, inner, other, nondefault = SCOPES[name]
    default = getattr(owner, attr)
    found = default if found_default else nondefault
    setattr(owner, attr, found)
    try:
        with scope(inner):                                   # a clean exit
            assert getattr(owner, attr) == inner
        assert getattr(owner, attr) is found or getattr(owner, attr) == found
        with pytest.raises(KeyError):                        # an exception
            with scope(inner):
                raise KeyError(name)
        assert getattr(owner, attr) is found or getattr(owner, attr) == found
        with scope(inner):                                   # nested inside itself with another value
            with scope(other):
                assert getattr(owner, attr) == other
            assert getattr(owner, attr) == inner
            with pytest.raises(KeyError):
                with scope(other):
                    raise KeyError(name)
            assert getattr(owner, attr) == inner
        assert getattr(owner, attr) is found or getattr(owner, attr) == found
    finally:
        setattr(owner, attr, default)


def test_onepass_scope_closes_a_stale_side_window_and_fresh_packs_empties_the_cache():
    dnn.SIDE_LIVE = 2                                        # (a backward pass that raised inside the window)
    with dnn.onepass_blocks(7):
        assert dnn.SIDE_LIVE == 0 and dnn.onepass_budget() == 7
    conv._PACK_CACHE['stale'] = None
    try:
        with conv.fresh_packs():
            assert not conv._PACK_CACHE
            conv._PACK_CACHE['packed inside'] = None
        assert not conv._PACK_CACHE
    finally:
        conv._PACK_CACHE.clear()


def test_batch_counting_around_a_failed_forward():
    bns = [dnn.BatchNorm2d(4) for _ in range(3)]
    count = lambda: [int(b.num_batches_tracked) for b in bns]      # noqa: E731
    with pytest.raises(ValueError):
        with dnn.deferred_batch_counts():
            bns[0]._count()
            bns[1]._count()
            raise ValueError('forward failed')
    assert dnn.BatchNorm2d._ran == [] and dnn.BatchNorm2d.count_batches is True and count() == [0, 0, 0]
    with dnn.deferred_batch_counts():
        bns[0]._count()                                      # noted in the failed body and again here: grows by 1, not 2
        bns[2]._count()
        dnn.count_batch(bns[2].num_batches_tracked)          # (the entry the GCN tail uses: a second batch of the same module)
        assert count() == [0, 0, 0] and len(dnn.BatchNorm2d._ran) == 3
    assert dnn.BatchNorm2d._ran == [] and count() == [1, 0, 2]
    bns[1]._count()                                          # outside a scope: counted at once
    assert count() == [1, 1, 2]


class _Stub(nn.Module):
    """What Trainer needs of a model, on the CPU: parameters, a BatchNorm2d whose counter the forward notes, `iuv2smpl.smpl`."""

    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(4, 2)
        self.bn = dnn.BatchNorm2d(2)
        self.iuv2smpl = types.SimpleNamespace(smpl=None)
        self.fail = False

    def forward(self, batch):
        self.bn._count()
        if self.fail:
            raise ValueError('forward failed')
        return {'losses': {'a': self.lin(batch['x']).pow(2).mean().reshape(1), 'b': self.lin.bias.sum().reshape(1)}}


def test_failed_step_leaves_the_trainer_usable():
    torch.manual_seed(0)
    model = _Stub()
    tr = trainer.Trainer(trainer.default_options(2), model=model, device=torch.device('cpu'), lr=1e-3, distributed=False)
    assert tr.store is None and tr.onepass_blocks == 0
    batch = {'x': torch.randn(3, 4)}
    rest = _resting()
    w0 = model.lin.weight.detach().clone()
    _, losses = tr.train_step(batch)                         # a good step runs: no library needed for empty weight-gradient queues
    assert set(losses) == {'a', 'b'} and not torch.equal(model.lin.weight, w0)
    assert int(model.bn.num_batches_tracked) == 1 and tr.step_count == 1 and _resting() == rest
    model.fail = True
    with pytest.raises(ValueError):
        tr.train_step(batch)
    assert _resting() == rest and int(model.bn.num_batches_tracked) == 1 and tr.step_count == 1
    model.fail = False
    tr.train_step(batch)
    assert int(model.bn.num_batches_tracked) == 2 and tr.step_count == 2 and _resting() == rest


def _walk(grouped):
    """Two steps of the _Net of test_distributed.py on a one-process CPU store with tiny buckets, a full backward pass inside
    backward_scope(True) each, then the walk: -> per step (callback arguments, issued_early, next_bucket())."""
    torch.manual_seed(5)
    net = _Net()
    st = GradStore(net.parameters(), bucket_mb=0.0002, device=torch.device('cpu'), world=1)
    x = torch.randn(6, 8)
    log = []
    for step in range(2):
        net.zero_grad(set_to_none=True)
        st.begin_step()
        st.backward_scope(True)
        net(x).pow(2).mean().backward()
        calls = []
        n = st.release_ready_group(lambda b0, b1: calls.append((b0, b1))) if grouped else st.release_ready(calls.append)
        log.append((calls, n, st.issued_early, st.next_bucket()))
        st.backward_scope(False)
    return st, net, log


def test_one_walk_one_reduce_on_the_host():
    st, net, single = _walk(False)
    _, _, group = _walk(True)
    nb = len(st.buckets)
    unused = min(st.bucket_of[id(p)] for p in net.unused.parameters())
    # the parent commit's GradStore on this net: four buckets, `unused` (registered last, so first in gradient-ready order) in bucket 0
    assert (nb, unused) == PARENT_WALK['layout']
    assert single == PARENT_WALK['single'] and group == PARENT_WALK['group']
    assert single[0][3] == unused                            # step 1 knows nothing yet and stops in front of the never-used module
    for (calls, n, early, nxt), (gcalls, gn, gearly, gnxt) in zip(single, group):
        assert (n, early, nxt) == (gn, gearly, gnxt) == (len(calls), len(calls), calls[-1] + 1 if calls else nxt)
        assert gcalls == ([(calls[0], calls[-1] + 1)] if calls else [])      # exactly the run released bucket by bucket
    assert st.release_ready(lambda bi: 1 / 0) == 0            # outside the backward pass: nothing to walk
    # one reduce body: without a process group neither form issues anything; the abort method forgets pending collectives
    st.reduce_bucket(0)
    st.reduce_buckets(0, nb)
    assert st.issued == [] and st._works == []
    st._works = [('work', 0, 4)]
    st.forget_pending()
    assert st._works == []


# (run once on the parent commit: the first step releases nothing, the second everything but the last bucket, which carries the mask)
PARENT_WALK = {'layout': (4, 0),
               'single': [([], 0, 0, 0), ([0, 1, 2], 3, 3, 3)],
               'group': [([], 0, 0, 0), ([(0, 3)], 3, 3, 3)]}


def test_abort_rule_drops_both_queues():
    job = lambda w: conv.WgradJob(0, w, None, None, (), None)      # noqa: E731
    w = nn.Parameter(torch.zeros(2, 2, 3, 3))
    try:
        conv._WQ.extend([job(w), job(w)])
        conv._WQG.extend([job(w), job(w)])
        conv.drop_wgrads()
        assert conv._WQ == [] and conv._WQG == []
        conv._WQ.extend([job(w), job(w)])
        conv._WQG.extend([job(w), job(w)])
        assert w.grad is None
        with pytest.raises(RuntimeError, match='copied or accumulated'):
            conv._check_adopted(conv._WQG[:1])
        assert conv._WQ == [] and conv._WQG == []
    finally:
        conv.drop_wgrads()
