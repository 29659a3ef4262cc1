"""Stream order of the vision-language training step (harness.Net.overlap_word_branch: the word branch on the library's caller lane).

The word branch -- Embed's word projection, ImageEncoder.fc_vis, the word-region scorer and their backward -- runs on a second stream
beside the chart.  An ordering mistake there does not crash: the lane reads memory its producer has not written yet (or that the current
stream has already handed to somebody else) and the step goes on with wrong VG scores.  These tests look for that where it happens:

  (a) the whole step against the float64 oracle at the input forms the reference trains with -- embedding widths 300 (GloVe) and 1324
      (w2v + ELMo), region features that are not fp32 or not a multiple of 16 wide, non-contiguous tokens -- with the lane on and off;
  (b) lane on against lane off, to the bit, while one stream is held back by a bounded sleep: a late producer on the current stream
      (every producer after the fork), or a late lane in the backward (the current stream reuses freed memory early).  The allocator is
      filled with NaN first, so that a read that comes too early sees NaN rather than the previous run's values;
  (c) the lane flags of one Net.forward are not inherited by a later direct call of the chart module;
  (d) the deferred embedding-table gradient (heads.DeferredTableGrads) keeps contributions that do not come through offer().

The skew cases keep the tokens contiguous: with the order broken, a non-contiguous token copy would be read on the lane as a gather
index before it is written, which is an out-of-bounds read rather than a wrong value.  Case (a) covers the non-contiguous tokens.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import grad_check

pytestmark = pytest.mark.gpu

V, D, B, L, K, R = 200, 48, 5, 6, 12, 36
C = L * (L + 1) // 2
LR = 2e-3
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'f64': torch.float64}


def _case(E, feat, dtype, tokens, seed=21):
    """A CLIORA Net (train mode, recorded dropout mask) and its batch.  tokens: 'contig' or 'strided' (a column slice of a wider tensor,
    the same values)."""
    from cliora_amd import harness as H
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(V, E)
    emb.weight.data.normal_(0.0, E ** -0.5)          # x = e mat^T (mat ~ N(0, 1)) of unit scale at every width
    net = H.build_net(D, emb, obj_feats=True, img_dim=feat, k_neg=K, vg_loss=True, use_contr=True)
    for p in net.img_encoder.parameters():
        torch.nn.init.normal_(p, std=0.05)
    net = net.cuda().train()
    g = torch.Generator().manual_seed(seed + 1)
    wide = torch.randint(0, V, (B, L + 3), generator=g)
    sent = wide[:, 2:2 + L]
    tok = wide.cuda()[:, 2:2 + L] if tokens == 'strided' else sent.contiguous().cuda()
    assert tok.is_contiguous() == (tokens == 'contig')
    feats = torch.relu(torch.randn(B, R, feat, generator=g)).to(DTYPES[dtype])
    neg = torch.randperm(V, generator=g)[:K]
    mask = (torch.rand(B, C, R, generator=g) > 0.1).float() / 0.9
    net.diora.dropout_mask = mask.cuda()
    bm = dict(sentences=tok, neg_samples=neg.cuda(), obj_feats=feats.cuda())
    cpu = dict(sentences=sent.contiguous(), neg_samples=neg, obj_feats=feats, mask=mask)
    return net, bm, cpu


# ---------------------------------------------------------------------------------------------------------------------------- (a)

def _oracle_losses(P, emb_w, cpu):
    """The step's three losses on the oracle (oracle/diora_ref.py), at the precision of P, with the recorded dropout mask."""
    from oracle import diora_ref as Rf
    mask = cpu['mask']
    xs, xw = Rf.embed_forward(emb_w, P['embed.mat'], P['embed.mat1'], cpu['sentences'])
    os_, ow = Rf.image_encoder_forward(P['img_encoder.fc.weight'], P['img_encoder.fc.bias'], P['img_encoder.fc_vis.weight'],
                                       P['img_encoder.fc_vis.bias'], cpu['obj_feats'])
    off = [C - (L - lv) * (L - lv + 1) // 2 for lv in range(L)] + [C]
    calls = [0]

    def replay(x, p, training):          # AttentionHead's dropout, level by level: the recorded mask
        i = calls[0]
        calls[0] += 1
        return x * mask[:, off[i]:off[i + 1]].to(x.dtype)
    orig = Rf.F.dropout
    Rf.F.dropout = replay
    try:
        chart = {k[len('diora.'):]: v for k, v in P.items() if k.startswith('diora.')}
        ref = Rf.diora_forward(chart, xs, xw, os_, ow, training=True)
    finally:
        Rf.F.dropout = orig
    assert calls[0] == L
    return {'reconstruct_softmax_loss': Rf.reconstruction_loss(emb_w, P['reconstruct_softmax_loss.mat'], cpu['sentences'], cpu['neg_samples'],
                                                               ref['outside_h']),
            'vg_loss': Rf.vg_loss(ref['vg_atten_score'], 1.0),
            'contrastive_loss': Rf.contrastive_loss(ref['inside_s'], ref['outside_s'], ref['all_atten_score'], 0.2, 1.0)}


# Every value of every axis, and every pair that involves E = 300 or non-fp32 features (E, feature width, feature dtype, tokens, lane)
PARITY_CASES = [
    (64, 32, 'f32', 'contig', True),
    (64, 32, 'f16', 'contig', True),
    (300, 40, 'f16', 'strided', False),
    (1324, 40, 'f16', 'strided', True),
    (64, 40, 'f64', 'strided', False),
    (300, 32, 'f64', 'contig', True),
    (1324, 32, 'f64', 'contig', False),
    (300, 40, 'f32', 'strided', True),
    (1324, 40, 'f32', 'contig', False),
]


@pytest.mark.parametrize('E,feat,dtype,tokens,overlap', PARITY_CASES,
                         ids=['E%d-F%d-%s-%s-%s' % (e, f, d, t, 'lane' if o else 'nolane') for e, f, d, t, o in PARITY_CASES])
def test_step_matches_the_fp64_oracle(E, feat, dtype, tokens, overlap, mfma_mode):
    """Losses, every parameter gradient of the first step and (E <= 300) the losses and parameters of three Trainer steps (clip 5.0 +
    Adam) against the oracle in float64 from the same parameters, mask and region features (fp16 features reach both sides as the same rounded values)."""
    from cliora_amd import harness as H
    net, bm, cpu = _case(E, feat, dtype, tokens)
    net.overlap_word_branch = overlap
    P = {k: p.detach().cpu().double().requires_grad_(True) for k, p in net.named_parameters() if p.requires_grad}
    emb_w = net.embed.embeddings.weight.detach().cpu().double()
    assert 'embed.embeddings.weight' not in P                         # frozen in a vision-language net (trainer.py:541)

    seen = []
    hook = net.diora.register_forward_pre_hook(lambda m, a: seen.append(m.word_lane is not None))
    out = net(bm['sentences'], bm['obj_feats'], bm['neg_samples'])
    hook.remove()
    assert seen == [overlap]
    ref = _oracle_losses(P, emb_w, cpu)
    assert list(ref) == net.loss_func_names
    for k, v in ref.items():
        assert abs(float(out[k].detach()) - float(v)) <= 1e-4 * max(1.0, abs(float(v))), (k, float(out[k].detach()), float(v))
    out.total().backward()
    sum(ref.values()).backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    for k, p in P.items():
        assert named[k].grad is not None, k
        grad_check(named[k].grad, p.grad, mfma_mode, 2e-4, k)
    g0 = {k: p.grad.detach().clone() for k, p in P.items()}
    err0 = {k: (named[k].grad.detach().cpu().double() - g0[k]).abs() for k in P}
    start = {k: p.detach().clone() for k, p in P.items()}

    if E > 300:
        # w2v + ELMo width: Adam divides each element's gradient by its own size, so over the 190 000 elements of the three E-wide
        # projections the elements whose gradient is at the fp32 rounding level move by a full lr in a direction the rounding picks;
        # their sum moves the third step's loss by ~4e-4 of itself (measured, the lane on and off alike), beyond the three-step
        # tolerances of test_net_losses_grads_and_three_adam_steps.  The first step above holds every loss and gradient here.
        return
    net.zero_grad()
    tr = H.Trainer(net, lr=LR)
    opt = torch.optim.Adam(list(P.values()), lr=LR, betas=(0.9, 0.999), eps=1e-8)
    for s in range(3):
        have = tr.step(bm, train=True)['total_loss']
        opt.zero_grad()
        want = sum(_oracle_losses(P, emb_w, cpu).values())
        want.backward()
        torch.nn.utils.clip_grad_norm_(list(P.values()), 5.0)
        opt.step()
        assert abs(have - float(want)) <= 2e-4 * max(1.0, abs(float(want))), (s, have, float(want))
    tol = 5e-4 if mfma_mode == 'f32' else 1e-3
    for k, p in P.items():
        have, want = named[k].detach().cpu().double(), p.detach()
        # Adam divides each gradient element by its own magnitude: an element whose true gradient is zero, or no larger than this
        # arithmetic's error on it, takes a step of up to lr in a direction the rounding picks.  Those are held to that walk's bound
        # from the start (test_gpu_harness.py::test_net_losses_grads_and_three_adam_steps), every other element to `tol`.
        noise = (g0[k].abs() < 1e-7) | (g0[k].abs() <= 10.0 * err0[k])
        assert float((have - start[k])[noise].abs().max() if noise.any() else 0.0) <= 3.2 * LR, k
        err = (have - want).abs()[~noise]
        assert float(err.max() if err.numel() else 0.0) <= tol * max(1.0, float(want.abs().max())), k


def test_word_branch_on_the_caller_lane_is_the_single_stream_step():
    """A vision-language training step with the word branch (Embed's word projection, ImageEncoder.fc_vis, the word-region scorer, their
    backward, the region matrix's half of the region-max backward) on the library's caller lane (harness.Net.overlap_word_branch,
    cliora_device_side_stream) against the same step on one stream: the same kernels on the same data, only the streams differ -- losses,
    every gradient of the first step and the parameters after three steps agree to the bit (sums of two terms commute)."""
    from cliora_amd import harness as H
    res = {}
    for overlap in (True, False):
        torch.manual_seed(21)
        V, E, D, B, L, K, R = 200, 64, 48, 5, 6, 12, 36
        net = H.build_net(D, torch.nn.Embedding(V, E), obj_feats=True, img_dim=32, k_neg=K, vg_loss=True, use_contr=True).cuda()
        for p in net.img_encoder.parameters():
            torch.nn.init.normal_(p, std=0.05)
        net.overlap_word_branch = overlap
        g = torch.Generator().manual_seed(22)
        bm = dict(sentences=torch.randint(0, V, (B, L), generator=g).cuda(), neg_samples=torch.randperm(V, generator=g)[:K].cuda(),
                  obj_feats=torch.randn(B, R, 32, generator=g).cuda())
        C = L * (L + 1) // 2
        net.diora.dropout_mask = (torch.rand(B, C, R, generator=g) > 0.1).float().cuda() / 0.9        # the same recorded mask in both runs
        net.train()
        seen = []
        hook = net.diora.register_forward_pre_hook(lambda m, a: seen.append(m.word_lane is not None))
        out = net(bm['sentences'], bm['obj_feats'], bm['neg_samples'])
        hook.remove()
        # the chart call ran with the lane exactly when the overlap is on; the module does not keep it (Net.forward resets the flags)
        assert seen == [overlap]
        assert net.diora.word_lane is None and not net.diora.word_inputs_on_lane
        out.total().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        net.zero_grad()
        tr = H.Trainer(net, lr=2e-3)
        losses = [tr.step(bm, train=True)['total_loss'] for _ in range(3)]
        res[overlap] = (float(out.total().detach()), grads, losses, {k: p.detach().clone() for k, p in net.named_parameters()})
    assert res[True][0] == res[False][0]
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) >= 10
    for k in res[False][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k
    assert res[True][2] == res[False][2]
    for k in res[False][3]:
        assert torch.equal(res[True][3][k], res[False][3][k]), k


# ---------------------------------------------------------------------------------------------------------------------------- (b)

@pytest.fixture(scope='module')
def sleep_cycles():
    """torch.cuda._sleep cycles for about 30 ms, measured here with events (bounded: at most 1e8 cycles whatever the measurement)."""
    c0 = 1_000_000
    torch.cuda._sleep(1000)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(c0)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    return int(min(100 * c0, max(c0, c0 * 30.0 / max(ms, 1e-3))))


def _poison(*numels):
    """Fill with NaN every free block of the small-allocation pool that the next fp32 tensors of these sizes could be given, then free
    them: a read of such a tensor before its producer wrote it sees NaN."""
    torch.cuda.synchronize()
    st = torch.cuda.memory_stats()
    free = st.get('reserved_bytes.small_pool.current', 0) - st.get('allocated_bytes.small_pool.current', 0)
    for n in sorted(set(numels), reverse=True):
        size = (n * 4 + 511) // 512 * 512
        keep = [torch.empty(n, device='cuda') for _ in range(min(4096, free // size + 2))]
        torch._foreach_mul_(keep, float('nan'))
        del keep
    torch.cuda.synchronize()


def _late_embed(net, cycles):
    """Net.embed, but every call first holds the current stream for `cycles`: every current-stream producer after the lane's fork --
    the token copy, the torch-path lookup, the fp32 conversion of the region features -- is late."""
    from cliora_amd import harness as H

    class LateEmbed(H.Embed):
        def forward(self, tokens, word_lane=None):
            torch.cuda._sleep(cycles)
            return super().forward(tokens, word_lane)
    net.embed.__class__ = LateEmbed


SKEW_CASES = [
    ('producer', 64, 32, 'f32'),
    ('producer', 64, 32, 'f16'),
    ('producer', 64, 32, 'f64'),
    ('producer', 64, 40, 'f32'),
    ('producer', 300, 32, 'f32'),
    ('producer', 1324, 32, 'f16'),
    ('lane', 64, 32, 'f32'),
    ('lane', 300, 40, 'f16'),
    ('both', 64, 32, 'f16'),
]


@pytest.mark.parametrize('skew,E,feat,dtype', SKEW_CASES, ids=['%s-E%d-F%d-%s' % c for c in SKEW_CASES])
def test_lane_on_is_bitwise_lane_off_under_stream_skew(skew, E, feat, dtype, sleep_cycles, monkeypatch):
    """The same kernels on the same data, only the streams differ: the losses of three Trainer steps, every gradient of the first step
    and the parameters after three steps agree to the bit, with a late current stream ('producer': a sleep at the start of Embed) or a
    late lane in the backward ('lane': a sleep at the head of every caller lane heads._step_lane hands out), or both."""
    from cliora_amd import harness as H
    from cliora_amd import heads
    if skew in ('lane', 'both'):
        orig = heads._step_lane

        def late_lane(device):
            lane = orig(device)
            if lane is not None:
                with torch.cuda.stream(lane):
                    torch.cuda._sleep(sleep_cycles)
            return lane
        monkeypatch.setattr(heads, '_step_lane', late_lane)
    res = {}
    for overlap in (True, False):
        net, bm, _ = _case(E, feat, dtype, 'contig')
        net.overlap_word_branch = overlap
        if skew in ('producer', 'both'):
            _late_embed(net, sleep_cycles)
        tr = H.Trainer(net, lr=LR)
        losses, grads = [], None
        for s in range(3):
            _poison(B * L * D, B * R * D, B * R * feat)
            losses.append(tr.step(bm, train=True)['total_loss'])
            if s == 0:
                grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        res[overlap] = (losses, grads, {k: p.detach().clone() for k, p in net.named_parameters()})
    assert all(x == x for x in res[False][0]), res[False][0]           # the single-stream step itself is finite
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) >= 10
    for k in res[False][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k
    for k in res[False][2]:
        assert torch.equal(res[True][2][k], res[False][2][k]), k


# ---------------------------------------------------------------------------------------------------------------------------- (c)

def test_lane_flags_do_not_outlive_the_forward(sleep_cycles):
    """After a Net.forward with the word branch on the lane, a direct call of the chart module in training mode with x_word made on the
    current stream behind a sleep scores what a fresh module scores, to the bit."""
    from cliora_amd.cliora import DioraMLP
    net, bm, _ = _case(64, 32, 'f32', 'contig')
    seen = []
    hook = net.diora.register_forward_pre_hook(lambda m, a: seen.append(m.word_lane is not None))
    net(bm['sentences'], bm['obj_feats'], bm['neg_samples'])
    hook.remove()
    assert seen == [True]
    assert net.diora.word_lane is None and not net.diora.word_inputs_on_lane
    fresh = DioraMLP(D, outside=True, normalize='unit', compress=False, share=True).cuda().train()
    fresh.load_state_dict(net.diora.state_dict())
    fresh.dropout_mask = net.diora.dropout_mask
    g = torch.Generator().manual_seed(5)
    x_span, x_src = torch.randn(B, L, D, generator=g).cuda(), torch.randn(B, L, D, generator=g).cuda()
    o_span, o_word = 0.3 * torch.randn(B, R, D, generator=g).cuda(), 0.3 * torch.randn(B, R, D, generator=g).cuda()

    def scores(m):
        _poison(B * L * D)
        torch.cuda._sleep(sleep_cycles)
        x_word = x_src * 1.0                         # made on the current stream, behind the sleep
        m(x_span, x_word, o_span, o_word)
        torch.cuda.synchronize()
        return m.vg_atten_score.detach().clone()
    have, want = scores(net.diora), scores(fresh)
    assert torch.isfinite(want).all()
    assert torch.equal(have, want)


# ---------------------------------------------------------------------------------------------------------------------------- (d)

@pytest.mark.parametrize('vl', [False, True])
def test_deferred_table_gradient_keeps_a_torch_autograd_producer(vl):
    """A torch-autograd lookup of the embedding table (F.embedding(tokens, w) @ P added to Embed's span output) besides the library's
    producers: the deferred flush must add its gradient, not overwrite it.  Defer on against defer off: the table gradient of the first
    step and the parameters after three steps, within test_gpu_heads.py::test_deferred_table_gradient_is_the_autograd_one's bounds."""
    from cliora_amd import harness as H

    class TorchTermEmbed(H.Embed):
        def forward(self, tokens, word_lane=None):
            span, word = super().forward(tokens, word_lane)
            return span + F.embedding(tokens, self.embeddings.weight) @ self.extra, word
    res = {}
    for defer in (True, False):
        torch.manual_seed(11)
        Vt, E, Dt, Bt, Lt, Kt = 300, 64, 48, 6, 7, 20
        emb = torch.nn.Embedding(Vt, E)
        net = H.build_net(Dt, emb, obj_feats=vl, img_dim=32, k_neg=Kt, vg_loss=vl, use_contr=vl).cuda()
        emb.weight.requires_grad = True
        net.embed.__class__ = TorchTermEmbed
        net.embed.extra = 0.2 * torch.randn(E, Dt, generator=torch.Generator().manual_seed(3)).cuda()
        if vl:
            for p in net.img_encoder.parameters():
                torch.nn.init.normal_(p, std=0.05)
        tr = H.Trainer(net, lr=LR)
        tr.defer_table_grads = defer
        g = torch.Generator().manual_seed(12)
        bm = dict(sentences=torch.randint(0, 40, (Bt, Lt), generator=g).cuda(), neg_samples=torch.randperm(Vt, generator=g)[:Kt].cuda())
        bm['neg_samples'][:3] = bm['sentences'][0, :3]
        if vl:
            bm['obj_feats'] = torch.randn(Bt, 36, 32, generator=g).cuda()
        net.train = lambda mode=True, net=net: torch.nn.Module.train(net, False)      # dropout off, as the existing deferred test
        snap = []
        update = tr.optimizer.step

        def step(*a, **k):                          # the table's gradient as the update receives it
            snap.append(emb.weight.grad.detach().clone())
            return update(*a, **k)
        tr.optimizer.step = step
        losses = [tr.step(bm, train=True)['total_loss'] for _ in range(3)]
        res[defer] = (losses, snap[0], {k: p.detach().clone() for k, p in net.named_parameters()})
    for a, b in zip(res[True][0], res[False][0]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b))
    a, b = res[True][1], res[False][1]
    assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    for k in res[False][2]:
        a, b = res[True][2][k], res[False][2][k]
        # img_encoder.fc_vis.bias has a true gradient of zero (the same vector added to every region cancels in the word-region
        # scorers): Adam walks it by up to lr per step on rounding noise, which the other order of the table sum changes -- held to
        # that walk's bound (test_gpu_harness.py::test_net_losses_grads_and_three_adam_steps)
        tol = 2 * 3.2 * LR if k == 'img_encoder.fc_vis.bias' else 2e-5 * max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= tol, k


@pytest.mark.parametrize('torch_term', [False, True])
def test_deferred_table_gradient_keeps_a_fifth_producer(torch_term):
    """Five library lookups of one table under one backward (cliora_rows_scatter_add_segments takes four: the fifth is refused by
    offer()), optionally with a torch-autograd lookup too, against the arena of a FlatGradAllReduce: the table's gradient after the
    flush is the float64 one, defer on and off."""
    from cliora_amd import heads, parallel
    Vt, Kt, Dt, n = 90, 64, 48, 30
    g = torch.Generator().manual_seed(8)
    w0 = torch.randn(Vt, Kt, generator=g)
    mats = [torch.randn(Dt, Kt, generator=g) for _ in range(6)]
    idx = [torch.randint(0, Vt, (n,), generator=g) for _ in range(6)]
    cots = [torch.randn(n, Dt, generator=g) for _ in range(6)]
    nlib = 5
    w64 = w0.double().requires_grad_(True)
    terms = [(F.embedding(idx[i], w64) @ mats[i].double().t() * cots[i].double()).sum() for i in range(nlib + int(torch_term))]
    sum(terms).backward()
    want = w64.grad
    W = torch.nn.Parameter(w0.cuda())
    arena = parallel.FlatGradAllReduce([W])
    got = {}
    try:
        for defer in (True, False):
            W.grad = None
            d = heads.DeferredTableGrads(arena) if defer else None
            heads._deferred, heads._step_lanes = d, set()
            try:
                loss = sum((heads.proj(W, idx[i].cuda(), mats[i].cuda()) * cots[i].cuda()).sum() for i in range(nlib))
                if torch_term:
                    loss = loss + (F.embedding(idx[nlib].cuda(), W) @ mats[nlib].cuda().t() * cots[nlib].cuda()).sum()
                loss.backward()
            finally:
                heads._deferred, heads._step_lanes = None, None
            if d is not None:
                assert len(d.pending[id(W)][2]) == 4
                d.flush()
            torch.cuda.synchronize()
            got[defer] = W.grad.detach().cpu().double()
    finally:
        arena.close()
    for defer, have in got.items():
        assert float((have - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), defer
    assert float((got[True] - got[False]).abs().max()) <= 2e-5 * max(1.0, float(got[False].abs().max()))
