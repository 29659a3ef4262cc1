#!/usr/bin/env python
"""Generate the golden fixtures in this directory by RUNNING THE REFERENCE.

Runs only in the build container (needs /root/reference on disk); the GPU box
never executes this.  Usage:  python tests/golden/make_golden.py

What is captured (inputs + expected outputs only -- no reference source):
  index_tables.npz   lidx/ridx/pidx/sidx for every (L <= 40, level)    [reference: net/inside_index.py, outside_index.py]
  diora_*.npz        DioraMLP charts, per-level hook scores, gradients  [net/diora.py]
  cliora_*.npz       cliora.DioraMLP (eval + train with recorded dropout masks), score tensors [net/cliora.py]
  net_*.npz          Net.forward losses + parameter grads, Trainer._step Adam updates [net/trainer.py]
  trees in diora_*/cliora_* files from analysis/cky.py + analysis/utils.py hooks
  sampler_batches.npz   FixedLengthBatchSampler batches, BatchIterator.partition  [data/dataloader.py, batch_iterator.py]
  interchange.npz + ref_model_*.pt   checkpoints written/loaded by Trainer.save_model/load_model, span lists, F1,
                        parse.jsonl trees  [net/trainer.py, analysis/utils.py, scripts/parse.py helpers]
  interchange_run.npz   the reference Net AFTER Trainer.load_model of ref_model_{noemb,ddp}.pt, run on a fixture batch:
                        charts, loss, trees (what a native module that loaded the same file must reproduce)
  shim_selection.npz    module name + state_dict keys of the chart module build_net constructs, --obj_feats off / on  [net/trainer.py]
"""
import os
import sys
import types
import json

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')
sys.modules.setdefault('cv2', types.ModuleType('cv2'))  # trainer.py:13 (visualization only)

from cliora.net import diora as ref_diora            # noqa: E402
from cliora.net import cliora as ref_cliora          # noqa: E402
from cliora.net import trainer as ref_trainer        # noqa: E402
from cliora.net.utils import ImageEncoder            # noqa: E402
from cliora.net.inside_index import get_inside_index      # noqa: E402
from cliora.net.outside_index import get_outside_index    # noqa: E402
from cliora.net.offset_cache import get_offset_cache      # noqa: E402
from cliora.analysis.cky import ParsePredictor            # noqa: E402
from cliora.analysis.utils import override_init_with_batch, override_inside_hook, get_actions, get_spans  # noqa: E402

torch.use_deterministic_algorithms(True)
torch.set_num_threads(4)
META = dict(torch=torch.__version__, numpy=np.__version__, threads=4)


def tree_to_str(t):
    return str(t)


def save(name, **arrs):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrs)
    print('wrote', name, os.path.getsize(path) // 1024, 'KiB')


def index_tables():
    out = {}
    for L in range(2, 41):
        off = get_offset_cache(L)
        out['off_%d' % L] = np.array([off[i] for i in range(L)], dtype=np.int32)
        li, ri, pi, si = [], [], [], []
        for level in range(1, L):
            a, b = get_inside_index(L, level, off)
            li.append(a.numpy()); ri.append(b.numpy())
        for level in range(L - 2, -1, -1):
            a, b = get_outside_index(L, level, off)
            pi.append(a.numpy()); si.append(b.numpy())
        out['lidx_%d' % L] = np.concatenate(li).astype(np.int16)
        out['ridx_%d' % L] = np.concatenate(ri).astype(np.int16)
        out['pidx_%d' % L] = np.concatenate(pi).astype(np.int16)   # levels L-2..0 concatenated
        out['sidx_%d' % L] = np.concatenate(si).astype(np.int16)
    save('index_tables.npz', **out)


def seeded_params(module, seed):
    g = torch.Generator().manual_seed(seed)
    for p in module.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g))


def state_np(module, prefix=''):
    return {prefix + k.replace('.', '__'): v.detach().numpy().copy() for k, v in module.state_dict().items()}


def attach_hooks(net):
    override_init_with_batch(net)
    override_inside_hook(net)


def run_cky(net, B, L):
    pp = ParsePredictor(net)
    trees = pp.parse_batch({'sentences': torch.zeros(B, L, dtype=torch.int64)})
    spans = [get_spans(get_actions(str(t).replace(',', ''))) for t in trees]
    return trees, spans


def diora_case(name, D, B, L, seed, share=True, normalize='unit', full=True, compress=False):
    torch.manual_seed(seed)
    net = ref_diora.DioraMLP(D, outside=True, normalize=normalize, compress=compress, share=share)
    seeded_params(net, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, L, D, generator=g).requires_grad_(True)
    cot = {k: torch.randn(s, generator=g) for k, s in
           [('inside_h', (B, L * (L + 1) // 2, D)), ('inside_s', (B, L * (L + 1) // 2, 1)),
            ('outside_h', (B, L * (L + 1) // 2, D)), ('outside_s', (B, L * (L + 1) // 2, 1))]}
    # pass 1: training-mode graph for gradients
    net.train()
    net(x, x)
    loss = sum((getattr(net, k) * v).sum() for k, v in cot.items())
    loss.backward()
    grads = {'grad__' + k.replace('.', '__'): p.grad.numpy().copy() for k, p in net.named_parameters()}
    grads['grad__x_span'] = x.grad.numpy().copy()
    charts = {k: getattr(net, k).detach().numpy().copy() for k in
              ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_c', 'outside_s')}
    # pass 2: hooks + CKY
    net.eval()
    attach_hooks(net)
    with torch.no_grad():
        net(x.detach(), x.detach())
    hook = {}
    for level in range(1, L):
        hook['hook_s_%d' % level] = torch.stack([net.saved_scalars[level][p] for p in range(L - level)], 1).numpy()
    trees, spans = run_cky(net, B, L)
    meta = dict(META, D=D, B=B, L=L, seed=seed, share=share, normalize=normalize, **({'compress': True} if compress else {}),
                trees=[tree_to_str(t) for t in trees], spans=[[list(s) for s in sp] for sp in spans])
    arrs = dict(meta=np.array(json.dumps(meta)))
    if full:
        arrs.update(state_np(net, 'param__'))
        arrs['x_span'] = x.detach().numpy()
        arrs.update({'cot__' + k: v.numpy() for k, v in cot.items()})
        arrs.update(charts)
        arrs.update(grads)
        arrs.update(hook)
    else:
        # large-D case: params / inputs / cotangents are regenerated from the seed by the test
        # (same torch build on the GPU box); store small exact slices + float64 checksums.
        C = L * (L + 1) // 2
        cells = np.array([0, L - 1, L, C // 2, C - 2, C - 1])
        arrs['cells'] = cells
        for k, v in charts.items():
            arrs[k + '__cells'] = v[:, cells]
            arrs[k + '__sum'] = np.array(v.astype(np.float64).sum())
            arrs[k + '__abssum'] = np.array(np.abs(v.astype(np.float64)).sum())
        arrs['inside_s'] = charts['inside_s']
        arrs['outside_s'] = charts['outside_s']
        for k, v in grads.items():
            arrs[k + '__sum'] = np.array(v.astype(np.float64).sum())
            arrs[k + '__abssum'] = np.array(np.abs(v.astype(np.float64)).sum())
            arrs[k + '__head'] = v.reshape(-1)[:64].copy()
        arrs.update(hook)
    save(name, **arrs)


class RecordingDropout(torch.nn.Module):
    """Same RNG draws as nn.Dropout(p) on an equally shaped input; keeps the masks."""

    def __init__(self, p):
        super().__init__()
        self.p = p
        self.masks = []

    def forward(self, x):
        if not self.training:
            return x
        m = torch.nn.functional.dropout(torch.ones_like(x), self.p, True)
        self.masks.append(m.detach().clone())
        return x * m


def cliora_case(name, D, B, L, seed, R=36):
    torch.manual_seed(seed)
    net = ref_cliora.DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
    seeded_params(net, seed)
    g = torch.Generator().manual_seed(seed + 1)
    C = L * (L + 1) // 2
    x_span = torch.randn(B, L, D, generator=g).requires_grad_(True)
    x_word = torch.randn(B, L, D, generator=g).requires_grad_(True)
    obj_span = (0.3 * torch.randn(B, R, D, generator=g)).requires_grad_(True)
    obj_word = (0.3 * torch.randn(B, R, D, generator=g)).requires_grad_(True)
    arrs = dict(x_span=x_span.detach().numpy(), x_word=x_word.detach().numpy(),
                obj_span=obj_span.detach().numpy(), obj_word=obj_word.detach().numpy())
    arrs.update(state_np(net, 'param__'))
    outs = ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_c', 'outside_s',
            'all_atten_score', 'vg_atten_score', 'atten_score')
    # --- eval mode (dropout off) + hooks + CKY
    net.eval()
    attach_hooks(net)
    with torch.no_grad():
        net(x_span.detach(), x_word.detach(), obj_span.detach(), obj_word.detach())
    for k in outs:
        arrs['eval__' + k] = getattr(net, k).detach().numpy().copy()
    trees, spans = run_cky(net, B, L)
    # --- training mode with recorded masks + gradients of the two VL losses
    net2 = ref_cliora.DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
    net2.load_state_dict(net.state_dict())
    net2.atten_head.dropout = RecordingDropout(0.1)
    net2.train()
    torch.manual_seed(seed + 2)
    net2(x_span, x_word, obj_span, obj_word)
    for k in outs:
        arrs['train__' + k] = getattr(net2, k).detach().numpy().copy()
    for i, m in enumerate(net2.atten_head.dropout.masks):
        arrs['mask_%d' % i] = m.numpy()
    sent = torch.zeros(B, L, dtype=torch.int64)
    lc, _ = ref_trainer.ContrastiveLoss(0.2, 1.0)(sent, net2)
    lv, _ = ref_trainer.VGLoss(1.0)(sent, net2.vg_atten_score)
    cot = {k: torch.randn(getattr(net2, k).shape, generator=g) for k in ('inside_h', 'outside_h')}
    total = lc + lv + sum((getattr(net2, k) * v).sum() for k, v in cot.items())
    total.backward()
    arrs['train__contrastive_loss'] = lc.detach().numpy()
    arrs['train__vg_loss'] = lv.detach().numpy()
    arrs.update({'cot__' + k: v.numpy() for k, v in cot.items()})
    for k, p in net2.named_parameters():
        arrs['grad__' + k.replace('.', '__')] = p.grad.numpy().copy()
    for k, t in (('x_span', x_span), ('x_word', x_word), ('obj_span', obj_span), ('obj_word', obj_word)):
        arrs['grad__' + k] = t.grad.numpy().copy()
    meta = dict(META, D=D, B=B, L=L, R=R, seed=seed, n_masks=len(net2.atten_head.dropout.masks),
                trees=[tree_to_str(t) for t in trees], spans=[[list(s) for s in sp] for sp in spans])
    arrs['meta'] = np.array(json.dumps(meta))
    save(name, **arrs)


def net_case(name, D, B, L, V, K, seed, vl):
    """Whole Net.forward + losses + Trainer._step (trainer.py:243-304, 450-455, 483-501)."""
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(V, 32)
    embed = ref_trainer.Embed(emb, input_size=32, size=D)
    enc = ImageEncoder(input_size=48, size=D)
    Diora = ref_cliora.DioraMLP if vl else ref_diora.DioraMLP
    d = Diora(D, outside=True, normalize='unit', compress=False, share=True)
    losses = [ref_trainer.ReconstructionSoftmaxLoss(emb, margin=1, k_neg=K, input_size=32, size=D)]
    if vl:
        emb.weight.requires_grad = False          # trainer.py:541
        losses += [ref_trainer.VGLoss(1.0), ref_trainer.ContrastiveLoss(0.2, 1.0)]
    net = ref_trainer.Net(embed, enc, d, obj_feats=vl, visualize=False, loss_funcs=losses)
    seeded_params(net, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(0.05 * torch.randn(p.shape, generator=g))   # reference zero-inits these (utils.py:45-50)
    sent = torch.randint(0, V, (B, L), generator=g)
    neg = torch.randperm(V, generator=g)[:K]
    obj = torch.randn(B, 36, 48, generator=g)
    arrs = dict(sentences=sent.numpy(), neg_samples=neg.numpy(), obj_feats=obj.numpy())
    arrs.update(state_np(net, 'param__'))
    bm = dict(example_ids=list(range(B)), sentences=sent, image_feats=torch.zeros(B, 1), neg_samples=neg,
              obj_feats=obj, boxes=torch.zeros(B, 36, 4), obj_cates=torch.zeros(B, 36), GT=None,
              batch_size=B, length=L)
    tr = ref_trainer.Trainer(net, k_neg=K, ngpus=1, cuda=False)
    tr.init_optimizer(torch.optim.Adam, dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8))
    net.eval()                                    # dropout off: deterministic whole-step parity
    out = tr.run_net(bm)
    arrs['total_loss'] = out['total_loss'].detach().numpy()
    tot = out['total_loss'].mean(dim=0).sum()
    tr.optimizer.zero_grad()
    tot.backward()
    for k, p in net.named_parameters():
        if p.grad is not None:
            arrs['grad__' + k.replace('.', '__')] = p.grad.numpy().copy()
    # three optimisation steps with the Trainer's own update (clip 5.0 + Adam), eval-mode dropout
    _train = net.train
    net.train = lambda *a, **k: _train(False)     # keep dropout off while exercising gradient_update
    steps = []
    for _ in range(3):
        r = tr._step(bm, train=True)
        steps.append(r['total_loss'])
    net.train = _train
    arrs['step_losses'] = np.array(steps, dtype=np.float64)
    arrs.update(state_np(net, 'after3__'))
    arrs['meta'] = np.array(json.dumps(dict(META, D=D, B=B, L=L, V=V, K=K, seed=seed, vl=vl, lr=2e-3)))
    save(name, **arrs)


def treelstm_case(name, D, B, L, seed, share=True):
    """RECONSTRUCTION, not tested reference behaviour: the TreeLSTM class exists in the reference only as
    commented-out text (cliora/net/vg.py:28-76).  Here that text is un-commented IN MEMORY, executed, and
    plugged into the live DioraBase skeleton (cliora/net/diora.py:205-450) the way the original DIORA did
    (inside/outside functions shared -- or, share=False, a second compose / score module for the outside pass as
    DioraMLP.init_parameters builds them, diora.py:459-464 -- and root_vector_out_c a parameter: the hint at
    diora.py:470-471).  Only inputs and outputs are stored."""
    import torch.nn as nn
    src = open('/root/reference/cliora/net/vg.py').read().split('\n')[27:76]
    code = '\n'.join(l[2:] if l.startswith('# ') else l.lstrip('#') for l in src)
    ns = {'nn': nn, 'torch': torch}
    exec(code, ns)
    TreeLSTM = ns['TreeLSTM']

    class DioraTreeLSTM(ref_diora.DioraBase):
        def init_parameters(self):
            self.inside_score_func = ref_diora.Bilinear(self.size)
            self.inside_compose_func = TreeLSTM(self.size, leaf=True)
            if self.share:
                self.outside_score_func = self.inside_score_func
                self.outside_compose_func = self.inside_compose_func
            else:
                self.outside_score_func = ref_diora.Bilinear(self.size)
                self.outside_compose_func = TreeLSTM(self.size)
            self.root_vector_out_h = nn.Parameter(torch.FloatTensor(self.size))
            self.root_vector_out_c = nn.Parameter(torch.FloatTensor(self.size))

    torch.manual_seed(seed)
    net = DioraTreeLSTM(D, outside=True, normalize='unit', compress=False, share=share)
    seeded_params(net, seed)
    g = torch.Generator().manual_seed(seed + 1)
    C = L * (L + 1) // 2
    x = torch.randn(B, L, D, generator=g).requires_grad_(True)
    keys = ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_c', 'outside_s')
    cot = {k: torch.randn((B, C, 1 if k.endswith('_s') else D), generator=g) for k in keys}
    net.train()
    net(x, x)
    sum((getattr(net, k) * v).sum() for k, v in cot.items()).backward()
    arrs = dict(x_span=x.detach().numpy())
    arrs.update(state_np(net, 'param__'))
    arrs.update({'cot__' + k: v.numpy() for k, v in cot.items()})
    arrs.update({k: getattr(net, k).detach().numpy().copy() for k in keys})
    seen = set()
    for k, p in net.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            arrs['grad__' + k.replace('.', '__')] = p.grad.numpy().copy()
    arrs['grad__x_span'] = x.grad.numpy().copy()
    net.eval()
    attach_hooks(net)
    with torch.no_grad():
        net(x.detach(), x.detach())
    trees, spans = run_cky(net, B, L)
    arrs['meta'] = np.array(json.dumps(dict(META, D=D, B=B, L=L, seed=seed, reconstruction=True, share=bool(share),
                                            trees=[tree_to_str(t) for t in trees])))
    save(name, **arrs)


def sampler_case(name):
    """Bucketed batching (cliora/data/dataloader.py:11-113) and rank partition (batch_iterator.py:53-66)
    on a synthetic corpus.  h5py is absent here; the module only needs it at import time."""
    sys.modules.setdefault('h5py', types.ModuleType('h5py'))
    from cliora.data.dataloader import FixedLengthBatchSampler
    from cliora.data.batch_iterator import BatchIterator

    class DS:          # what the sampler touches: len(ds) and ds.dataset[i]
        def __init__(self, sents):
            self.dataset = sents

        def __len__(self):
            return len(self.dataset)

    rs = np.random.RandomState(5)
    lengths = rs.randint(3, 41, size=600)
    sents = [[0] * int(n) for n in lengths]
    arrs = dict(lengths=lengths.astype(np.int32))
    cases = [dict(batch_size=16, include_partial=False, maxlen=None, length_to_size=None, seed=11),
             dict(batch_size=16, include_partial=True, maxlen=30, length_to_size=None, seed=3),
             dict(batch_size=32, include_partial=True, maxlen=None, length_to_size={10: 16, 25: 4}, seed=7)]
    for ci, c in enumerate(cases):
        s = FixedLengthBatchSampler(DS(sents), c['batch_size'], include_partial=c['include_partial'],
                                    rng=np.random.RandomState(c['seed']), maxlen=c['maxlen'], length_to_size=c['length_to_size'])
        flat, sizes = [], []
        for _epoch in range(2):                      # the rng carries over between epochs
            for b in s:
                flat += list(b)
                sizes.append(len(b))
        arrs['case%d_flat' % ci] = np.array(flat, dtype=np.int32)
        arrs['case%d_sizes' % ci] = np.array(sizes, dtype=np.int32)
    # rank partition of tensors and lists
    bi = BatchIterator.__new__(BatchIterator)
    t = torch.arange(22).view(11, 2)
    lst = list(range(100, 111))
    for world in (2, 4):
        for rank in range(world):
            arrs['part_t_%d_%d' % (world, rank)] = bi.partition(t, rank, range(world)).numpy()
            arrs['part_l_%d_%d' % (world, rank)] = np.array(bi.partition(lst, rank, range(world)), dtype=np.int32)
    arrs['meta'] = np.array(json.dumps(dict(META, cases=[{k: (v if not isinstance(v, dict) else {str(a): b for a, b in v.items()}) for k, v in c.items()} for c in cases])))
    save(name, **arrs)


def _parse_helpers():
    """The tree helpers of cliora/scripts/parse.py:20-98, executed from its text: the module itself needs torchvision
    and the training CLI at import time."""
    import ast
    src = open('/root/reference/cliora/scripts/parse.py').read()
    mod = ast.parse(src)
    keep = [n for n in mod.body if (isinstance(n, ast.FunctionDef) and n.name in ('remove_using_flat_mask', 'flatten_tree', 'postprocess', 'replace_leaves'))
            or (isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', '') == 'punctuation_words')]
    ns = {}
    exec(compile(ast.Module(body=keep, type_ignores=[]), 'parse.py', 'exec'), ns)
    return ns


def interchange_case(name):
    """Checkpoint files written / read by the reference's Trainer, span lists, F1 numbers and parse.jsonl trees."""
    import copy
    import collections
    from cliora.analysis.utils import get_stats
    torch.manual_seed(5)
    D, V, K = 24, 41, 6

    def make_net(seed, vl):
        emb = torch.nn.Embedding(V, 16)
        embed = ref_trainer.Embed(emb, input_size=16, size=D)
        enc = ImageEncoder(input_size=20, size=D)
        Diora = ref_cliora.DioraMLP if vl else ref_diora.DioraMLP
        d = Diora(D, outside=True, normalize='unit', compress=False, share=True)
        losses = [ref_trainer.ReconstructionSoftmaxLoss(emb, margin=1, k_neg=K, input_size=16, size=D)]
        net = ref_trainer.Net(embed, enc, d, obj_feats=vl, visualize=False, loss_funcs=losses)
        seeded_params(net, seed)
        return net

    arrs = {}
    src = make_net(61, False)
    tr = ref_trainer.Trainer(src, k_neg=K, ngpus=1, cuda=False)
    tr.save_model(False, os.path.join(HERE, 'ref_model_noemb.pt'))
    tr.save_model(True, os.path.join(HERE, 'ref_model_emb.pt'))
    # what a DistributedDataParallel-wrapped net saves: every key behind 'module.', plus a key no net has
    sd = collections.OrderedDict(('module.' + k, v) for k, v in src.state_dict().items())
    sd['module.not_a_parameter'] = torch.zeros(3)
    torch.save({'state_dict': sd}, os.path.join(HERE, 'ref_model_ddp.pt'))
    arrs.update(state_np(src, 'src__'))
    for tag, fname, origin_emb in (('noemb', 'ref_model_noemb.pt', False), ('emb', 'ref_model_emb.pt', True), ('ddp', 'ref_model_ddp.pt', True)):
        dst = make_net(67, False)
        if tag == 'noemb':
            arrs.update(state_np(dst, 'dst0__'))
        ref_trainer.Trainer.load_model(origin_emb, dst, os.path.join(HERE, fname))
        arrs.update(state_np(dst, 'loaded_%s__' % tag))
    # trees: random binary bracketings, spans / F1 / post-processing by the reference's own helpers
    ph = _parse_helpers()
    rs = np.random.RandomState(3)

    def rand_tree(lo, hi):
        if hi - lo == 1:
            return lo
        k = rs.randint(lo + 1, hi)
        return (rand_tree(lo, k), rand_tree(k, hi))

    words = ['a', 'b', 'the', 'dog', ',', 'runs', '.', 'fast', '?', 'x1', '-LRB-', 'y', '!', 'z']
    cases, corpus, sent_f1 = [], [0., 0., 0.], []
    for n in (2, 3, 5, 8, 11, 14):
        for _rep in range(3):
            t, gold_t = rand_tree(0, n), rand_tree(0, n)
            toks = [words[int(i)] for i in rs.randint(0, len(words), size=n)]
            if _rep == 1:
                toks[-1] = '.'
            spans = get_spans(get_actions(str(t)))
            gold = set(get_spans(get_actions(str(gold_t)))[:-1]) if _rep != 2 else set()
            pred = set(spans[:-1])
            tp, fp, fn = get_stats(pred, gold)
            corpus[0] += tp; corpus[1] += fp; corpus[2] += fn
            overlap = pred.intersection(gold)
            prec = float(len(overlap)) / (len(pred) + 1e-8)
            reca = float(len(overlap)) / (len(gold) + 1e-8)
            if len(gold) == 0:
                reca = 1.
                if len(pred) == 0:
                    prec = 1.
            sent_f1.append(2 * prec * reca / (prec + reca + 1e-8))
            leaves = ph['replace_leaves'](copy.deepcopy(t), toks)
            cases.append(dict(tree=t, tokens=toks, spans=spans, gold=sorted(gold), replaced=leaves,
                              post=ph['postprocess'](copy.deepcopy(leaves), toks), flat=ph['flatten_tree'](t)))
    tp, fp, fn = corpus
    prec, rec = tp / (tp + fp), tp / (tp + fn)
    arrs['meta'] = np.array(json.dumps(dict(META, D=D, V=V, K=K, cases=cases, corpus_f1=2 * prec * rec / (prec + rec),
                                            sent_f1=float(np.mean(np.array(sent_f1))))))
    save(name, **arrs)


def interchange_run_case(name):
    """The reference's own Net after Trainer.load_model (trainer.py:399-435) of the checkpoints interchange_case wrote, run forward on a
    fixture batch (trainer.py:243-304): the charts, the loss and the trees a native module that loaded the same file must reproduce."""
    D, V, K, B, L = 24, 41, 6, 3, 7

    def make_net(seed):
        emb = torch.nn.Embedding(V, 16)
        embed = ref_trainer.Embed(emb, input_size=16, size=D)
        enc = ImageEncoder(input_size=20, size=D)
        d = ref_diora.DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
        losses = [ref_trainer.ReconstructionSoftmaxLoss(emb, margin=1, k_neg=K, input_size=16, size=D)]
        net = ref_trainer.Net(embed, enc, d, obj_feats=False, visualize=False, loss_funcs=losses)
        seeded_params(net, seed)
        return net

    g = torch.Generator().manual_seed(71)
    sent = torch.randint(0, V, (B, L), generator=g)
    neg = torch.randperm(V, generator=g)[:K]
    bm = dict(example_ids=list(range(B)), sentences=sent, image_feats=torch.zeros(B, 1), neg_samples=neg, obj_feats=None,
              boxes=torch.zeros(B, 36, 4), obj_cates=torch.zeros(B, 36), GT=None, batch_size=B, length=L)
    arrs = dict(sentences=sent.numpy(), neg_samples=neg.numpy())
    arrs.update(state_np(make_net(67), 'dst0__'))          # the receiving net's own initialisation (the embedding table survives a noemb load)
    for tag, fname, origin_emb in (('noemb', 'ref_model_noemb.pt', False), ('ddp', 'ref_model_ddp.pt', True)):
        net = make_net(67)
        ref_trainer.Trainer.load_model(origin_emb, net, os.path.join(HERE, fname))
        net.eval()
        tr = ref_trainer.Trainer(net, k_neg=K, ngpus=1, cuda=False)
        attach_hooks(net.diora)
        with torch.no_grad():
            out = tr.run_net(bm)
        d = net.diora
        for k in ('inside_h', 'inside_s', 'outside_h', 'outside_s'):
            arrs['%s__%s' % (tag, k)] = getattr(d, k).detach().numpy().copy()
        arrs['%s__total_loss' % tag] = out['total_loss'].detach().numpy().copy()
        arrs['%s__trees' % tag] = np.array(json.dumps([tree_to_str(t) for t in run_cky(net.diora, B, L)[0]]))
    arrs['meta'] = np.array(json.dumps(dict(META, D=D, V=V, K=K, B=B, L=L)))
    save(name, **arrs)


def shim_selection_case(name):
    """The chart module the reference's own build_net constructs (trainer.py:518-526, 552) for --obj_feats off / on: its
    module name and state_dict keys, so tests/test_selection_shim.py can check the shim's selection without the reference."""
    import argparse
    arrs = {}
    for obj_feats in (False, True):
        opt = argparse.Namespace(lr=1e-3, hidden_dim=16, k_neg=3, normalize='unit', cuda=False, local_rank=0, share=True, arch='mlp',
                                 obj_feats=obj_feats, multigpu=False, emb='none', margin=1.0, vl_margin=0.2, hinge_margin=1.0,
                                 alpha_contr=1.0, vg_loss=obj_feats, alpha_vg=1.0, use_contr=obj_feats, use_contr_ce=False,
                                 visualize=False, load_model_path=None, experiment_name='shim-fixture')
        diora = ref_trainer.build_net(opt, torch.nn.Embedding(20, 8)).net.diora
        tag = 'vl' if obj_feats else 'text'
        arrs['module__' + tag] = np.array(type(diora).__module__)
        arrs['keys__' + tag] = np.array(sorted(diora.state_dict()))
    save(name, meta=np.array(json.dumps(META)), **arrs)


if __name__ == '__main__':
    if sys.argv[1:] == ['interchange_run']:          # one new fixture without rewriting the others
        interchange_run_case('interchange_run.npz')
        sys.exit(0)
    if sys.argv[1:] == ['shim_selection']:
        shim_selection_case('shim_selection.npz')
        sys.exit(0)
    index_tables()
    diora_case('diora_c1.npz', D=50, B=8, L=10, seed=1234)                       # BASELINE config 1
    diora_case('diora_noshare.npz', D=24, B=3, L=7, seed=7, share=False)
    # diora.py:342-343 (never enabled by trainer.py:552).  With compress every gradient depends on every ReLU through the root, so the
    # seed is one whose second-layer pre-activations all stay 7e-5 of their scale away from zero (seed 19 has one at 1.5e-7: the
    # split-bf16 mode lands on the other side of that kink and every gradient of the 24-d case moves by 1e-4 .. 4e-3)
    diora_case('diora_compress.npz', D=24, B=3, L=7, seed=21, compress=True)
    diora_case('diora_nonorm.npz', D=16, B=2, L=5, seed=9, normalize='none')
    diora_case('diora_len2.npz', D=20, B=2, L=2, seed=11)
    diora_case('diora_c2_small.npz', D=400, B=2, L=20, seed=1234, full=False)    # config 2 shape, B=2
    cliora_case('cliora_small.npz', D=50, B=4, L=8, seed=21)                     # config 3 shape, small
    net_case('net_diora.npz', D=40, B=4, L=6, V=97, K=10, seed=31, vl=False)
    net_case('net_cliora.npz', D=40, B=4, L=6, V=97, K=10, seed=33, vl=True)
    treelstm_case('treelstm_recon.npz', D=24, B=3, L=7, seed=41)
    treelstm_case('treelstm_recon_noshare.npz', D=24, B=3, L=7, seed=43, share=False)
    sampler_case('sampler_batches.npz')
    interchange_case('interchange.npz')
    interchange_run_case('interchange_run.npz')
    shim_selection_case('shim_selection.npz')
