"""RecognitionLattice.align_expectation on the GPU (lt_table_align_expectation
and lt_table_string_scatter, lt_align_expect.hip) against the float64
reference of tests/align_expect_ref.py (double autograd of
cpu._string_distance in Log), at the kernel's lane and slice boundaries
(U = 63 .. 255), the LDS rule's boundaries for P = 1, 2, 4 (the last T whose
history fits LDS and the first that goes to the workspace: 210 / 211, 103 /
104, 50 / 51; include/lt_string_expect.h), a trigram with epsilons, random
next-state tables (one too large to stage in LDS), a transcript of one
repeated pair (most positions share cells), num_labels 0 and U, num_frames
0, 1, 2 and odd and even midpoints, -inf arcs with NaN values under them, bf16
weights, and the two shapes past the kernel's range (the on-device
restatement).

Bounds (none invented here).
* expected and log_prob: rtol = atol = 1e-4, the project's Log parity bound.
* emission and blank_occ: the same reference run in float32 is the yardstick:
  its max abs error against the float64 run on the same inputs, per array,
  computed at run time; the kernel may err by at most 4x that (a different
  summation order and the hardware exp / log), as in test_gpu_align_post.py.
* cov_lex, cov_blank and the dense dW: 4x the yardstick's error on that array,
  and never tighter than the posterior bound (4x the larger of the two
  posterior yardsticks), as in test_gpu_expectation.py.
* a sum of n terms may miss its exact value by n times the terms' bound.
Every figure is printed before it is asserted (pytest -s shows them;
profiles/align_expect_parity.txt keeps the table).
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from last_torch_amd import cpu
from last_torch_amd import lattices
import align_expect_ref as ref
import poisoned_buffers

pytestmark = pytest.mark.gpu

FACTOR = 4.0  # kernel error <= FACTOR * the float32 yardstick's error
MINUS_INF_SALT = 'seed-98'  # picked on the CPU: every utterance but the pathless one stays aligned

CASES = [
    # name, V, n (FullNGram) or None (random table of C states), C, T, U, dtype, labels
    ('bigram_u63', 32, 1, None, 70, 63, 'f32', 'random'),
    ('bigram_u64', 32, 1, None, 70, 64, 'f32', 'random'),   # P 1 -> 2
    ('bigram_u65', 32, 1, None, 70, 65, 'f32', 'random'),
    ('bigram_u127', 32, 1, None, 70, 127, 'f32', 'random'),
    ('bigram_u128', 32, 1, None, 70, 128, 'f32', 'random'),  # P 2 -> 4
    ('bigram_u255_t260', 32, 1, None, 260, 255, 'f32', 'random'),
    # the LDS rule: 36 SP + 12 SP T <= 160 KiB, SP = 64 P
    ('p1_u20_t210_lds', 8, 1, None, 210, 20, 'f32', 'random'),
    ('p1_u20_t211_ws', 8, 1, None, 211, 20, 'f32', 'random'),
    ('p1_u20_t210_lds_bf16', 8, 1, None, 210, 20, 'bf16', 'random'),
    ('p1_u20_t211_ws_bf16', 8, 1, None, 211, 20, 'bf16', 'random'),
    ('p2_u100_t103_lds', 8, 1, None, 103, 100, 'f32', 'random'),
    ('p2_u100_t104_ws', 8, 1, None, 104, 100, 'f32', 'random'),
    ('p2_u100_t103_lds_bf16', 8, 1, None, 103, 100, 'bf16', 'random'),
    ('p2_u100_t104_ws_bf16', 8, 1, None, 104, 100, 'bf16', 'random'),
    ('p4_u130_t50_lds', 8, 1, None, 50, 130, 'f32', 'random'),
    ('p4_u130_t51_ws', 8, 1, None, 51, 130, 'f32', 'random'),
    ('p4_u130_t50_lds_bf16', 8, 1, None, 50, 130, 'bf16', 'random'),
    ('p4_u130_t51_ws_bf16', 8, 1, None, 51, 130, 'bf16', 'random'),
    ('trigram_v5_eps', 5, 2, None, 30, 9, 'f32', 'epsilons'),
    ('table_c17_v6', 6, None, 17, 30, 9, 'f32', 'epsilons'),
    ('table_c300_v28', 28, None, 300, 20, 9, 'f32', 'epsilons'),  # too large to stage in LDS
    ('repeated_pair', 4, 1, None, 40, 24, 'f32', 'pair'),
    ('nl_0_and_u', 6, 1, None, 30, 12, 'f32', 'nl_edges'),
    ('mixed_nf', 6, 1, None, 33, 9, 'f32', 'mixed_nf'),
    ('minus_inf', 4, 1, None, 12, 3, 'f32', 'minus_inf'),
]
_BY_NAME = {c[0]: c for c in CASES}
_PROBLEMS = {}


def _context(rng, V, n, C):
  if n is not None:
    return lt.contexts.FullNGram(vocab_size=V, context_size=n)
  return lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))


def _problem(name, variant=''):
  """A dict of host tensors: the inputs of a case, the float64 reference (r64)
  and the float32 yardstick's errors (err), computed once and shared by the
  tests that use it (nothing changes them)."""
  key = name + variant
  if key in _PROBLEMS:
    return _PROBLEMS[key]
  _, V, n, C, T, U, dt, kind = _BY_NAME[name]
  salt = MINUS_INF_SALT if kind == 'minus_inf' else ''
  rng = np.random.default_rng(zlib.crc32((key + salt).encode()))
  ctx = _context(rng, V, n, C)
  nf = [T, T - 3, 1, 0]
  nl = [min(U, T), max(0, min(U, T - 3) - 2), 1, 0]
  if kind == 'nl_edges':
    nl = [0, U, 1, 0]
  if kind == 'mixed_nf':
    nf, nl = [0, 1, 2, 3, 15, 16, 17, 33], [0, 1, 2, 2, 9, 9, 8, 9]
  if kind == 'minus_inf':
    nf, nl = nf + [T], nl + [U]
  B = len(nf)
  W = rng.standard_normal((B, T, ctx.shape()[0], V + 1)).astype(np.float32)
  lab = rng.integers(0 if kind == 'epsilons' else 1, V + 1, (B, U)).astype(np.int32)
  if kind == 'pair':
    lab[:] = np.tile([1, 2], U // 2 + 1)[:U]
    lab[1] = np.tile([3, 3, 1], U // 3 + 1)[:U]
  lv = rng.standard_normal((B, T, U)).astype(np.float32)
  bv = rng.standard_normal((B, T, U + 1)).astype(np.float32)
  if kind == 'minus_inf':
    W[rng.random(W.shape) < 0.3] = -np.inf
    W[4, 0, 0, :] = -np.inf  # nothing leaves the start state: no path at all
  W, lab, lv, bv = torch.tensor(W), torch.tensor(lab), torch.tensor(lv), torch.tensor(bv)
  if dt == 'bf16':
    W = W.bfloat16().float()
  nf, nl = torch.tensor(nf, dtype=torch.int32), torch.tensor(nl, dtype=torch.int32)
  if kind == 'minus_inf':  # NaN under every -inf arc: never read into the arithmetic
    blank, lex = cpu.string_weights(W, lab.long(), ctx)
    lv[~torch.isfinite(lex)] = torch.nan
    bv[~torch.isfinite(blank)] = torch.nan
  r64, err = ref.yardstick(W, nf, lab, nl, ctx, lv, bv)
  fin = torch.isfinite(r64['log_prob'])
  if kind == 'minus_inf' and not variant:
    assert fin.tolist() == [True, True, True, True, False]
    assert (r64['emission'][:3].sum((1, 2)) > 0).all()
  elif kind != 'minus_inf':
    assert fin.all()
  p = dict(name=name, ctx=ctx, W=W, nf=nf, nl=nl, lab=lab, lv=lv, bv=bv, dt=dt, r64=r64, err=err,
           fin=fin, post_bound=FACTOR * max(err['emission'], err['blank_occ']))
  _PROBLEMS[key] = p
  return p


def _bound(p, key):
  """The bound of a covariance / dense-gradient array."""
  return max(FACTOR * p['err'][key], p['post_bound'])


def _dev(p, cuda):
  W = p['W'].to(cuda)
  if p['dt'] == 'bf16':
    W = W.bfloat16()
  graph = ref.lattice(p['ctx'], 0, p['W'].to(cuda))._graph(cuda)
  return graph, W.contiguous(), {k: p[k].to(cuda) for k in ('nf', 'lab', 'nl', 'lv', 'bv')}


def _expect(graph, W, d, **kw):
  return nat.table_align_expectation(graph, W, d['lv'], d['bv'], d['nf'], d['lab'], d['nl'], **kw)


def _scatter(graph, W, d, g_lex, g_blank):
  return nat.table_string_scatter(graph, W, g_lex, g_blank, d['nf'], d['lab'], d['nl'])


def _err(got, want):
  return float((got.double().cpu() - want).abs().max()) if want.numel() else 0.0


def _check_values(p, E, lp):
  E, lp = E.double().cpu(), lp.double().cpu()
  fin, r64 = p['fin'], p['r64']
  assert torch.isfinite(E).all() and not torch.isnan(lp).any()
  assert torch.equal(torch.isfinite(lp), fin) and (lp[~fin] == -torch.inf).all()
  assert (E[~fin] == 0).all()
  print(f"\n{p['name']}: expected {_err(E, r64['expected']):.3g} log_prob "
        f"{_err(lp[fin], r64['log_prob'][fin]):.3g}", end='')
  np.testing.assert_allclose(E.numpy(), r64['expected'].numpy(), rtol=1e-4, atol=1e-4)
  np.testing.assert_allclose(lp[fin].numpy(), r64['log_prob'][fin].numpy(), rtol=1e-4, atol=1e-4)


def _check_arrays(p, em, bo, cl, cb):
  """Parity, exact zeros and the invariants of the four string-coordinate arrays."""
  r64, err, fin = p['r64'], p['err'], p['fin']
  nf, nl = p['nf'].tolist(), p['nl'].tolist()
  B, T, U = r64['emission'].shape
  got = dict(emission=em, blank_occ=bo, cov_lex=cl, cov_blank=cb)
  for k, x in got.items():
    assert x.dtype == torch.float32 and tuple(x.shape) == tuple(r64[k].shape)
    got[k] = x = x.cpu()
    assert torch.isfinite(x).all(), k
    for b in range(B):
      n = max(min(nl[b], U), 0)
      lexical = k in ('emission', 'cov_lex')
      assert (x[b, max(nf[b], 0):] == 0).all() and (x[b, :, n + (0 if lexical else 1):] == 0).all()
      if not fin[b]:
        assert (x[b] == 0).all()
  bounds = dict(emission=FACTOR * err['emission'], blank_occ=FACTOR * err['blank_occ'],
                cov_lex=_bound(p, 'cov_lex'), cov_blank=_bound(p, 'cov_blank'))
  figs = {k: _err(got[k], r64[k]) for k in got}
  print(' | ' + ' | '.join(f'{k} {figs[k]:.3g} / {err[k]:.3g}' for k in got), end='')
  col = fr = cv = 0.0
  for b in range(B):
    if not fin[b] or nf[b] <= 0:
      continue
    e, o = got['emission'][b, :nf[b]].double(), got['blank_occ'][b, :nf[b]].double()
    if nl[b] > 0:
      col = max(col, float((e[:, :nl[b]].sum(0) - 1).abs().max()))
    fr = max(fr, float((e.sum(1) + o.sum(1) - 1).abs().max()))
    cv = max(cv, float((got['cov_lex'][b, :nf[b]].double().sum(1) +
                        got['cov_blank'][b, :nf[b]].double().sum(1)).abs().max()))
  print(f' | column sums off 1 by {col:.3g}, frame sums by {fr:.3g}, frame covariance sums off 0 '
        f'by {cv:.3g}', end='')
  for k in got:
    assert figs[k] <= bounds[k], (k, figs[k], bounds[k])
  arcs = 2 * max(nl) + 1  # arcs of a frame that carry weight
  assert col <= bounds['emission'] * T, (col, bounds['emission'], T)
  assert fr <= p['post_bound'] * arcs, (fr, p['post_bound'], arcs)
  assert cv <= max(bounds['cov_lex'], bounds['cov_blank']) * arcs, (cv, arcs)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_both_abi_calls_and_the_public_method_match_the_reference(cuda, name):
  p = _problem(name)
  r64, err = p['r64'], p['err']
  graph, W, d = _dev(p, cuda)
  assert nat.table_align_expectation_supported(graph, W, d['lab'])
  nbytes = ctypes.c_size_t(0)
  pb = nat._tproblem(graph, W, d['lab'].shape[-1])
  nat._check(nat.lib().lt_table_align_expectation_workspace_bytes(
      ctypes.byref(graph.g), ctypes.byref(pb), ctypes.byref(nbytes)), 'query')
  if '_lds' in name or '_ws' in name:
    assert (nbytes.value > 0) == ('_ws' in name)
  E, lp, em, bo, cl, cb = _expect(graph, W, d)
  _check_values(p, E, lp)
  _check_arrays(p, em, bo, cl, cb)
  # emission is lt_table_align_posteriors' output
  em2, lp2 = nat.table_align_posteriors(graph, W, d['nf'], d['lab'], d['nl'])
  k_p = _err(em, em2.double().cpu())
  print(f' | emission vs lt_table_align_posteriors {k_p:.3g}', end='')
  assert k_p <= FACTOR * err['emission'] and torch.equal(torch.isfinite(lp), torch.isfinite(lp2))
  # the scatter of the covariances is d expected / dW, of the posteriors d log_prob / dW
  dwe, dwl = _scatter(graph, W, d, cl, cb), _scatter(graph, W, d, em, bo)
  assert dwe.dtype == torch.float32 and tuple(dwe.shape) == tuple(W.shape)
  k_e, k_l = _err(dwe, r64['dW_expected']), _err(dwl, r64['dW_log_prob'])
  print(f" | dW_expected {k_e:.3g} / {err['dW_expected']:.3g} | dW_log_prob {k_l:.3g} / "
        f"{err['dW_log_prob']:.3g}", end='')
  assert k_e <= _bound(p, 'dW_expected') and k_l <= _bound(p, 'dW_log_prob')
  live = (torch.arange(W.shape[1])[None] < p['nf'][:, None]) & p['fin'][:, None]
  assert not dwe.cpu()[~live].any() and not dwl.cpu()[~live].any()
  if p['dt'] == 'bf16':
    return  # TableWeightFn hands out fp32: the bf16 kernels through the bindings only
  # the public method, with autograd
  g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
  B = len(p['nf'])
  a, b = torch.randn([B], generator=g), torch.randn([B], generator=g)
  table = p['W'].to(cuda).requires_grad_(True)
  lv, bv = d['lv'].clone().requires_grad_(True), d['bv'].clone().requires_grad_(True)
  lat = ref.lattice(p['ctx'], 0, table)
  E, lp = lat.align_expectation(ref.frames((B,), W.shape[1], cuda), d['nf'], d['lab'], d['nl'], lv,
                                bv)
  assert E.device == cuda and lp.device == cuda and E.requires_grad and lp.requires_grad
  _check_values(p, E.detach(), lp.detach())
  loss = (a.to(cuda) * E + b.to(cuda) * torch.where(torch.isfinite(lp), lp,
                                                   torch.zeros_like(lp))).sum()
  dW, dl, db = torch.autograd.grad(loss, [table, lv, bv], retain_graph=True)
  ad, bd = a.double(), b.double()
  e4 = lambda x: x[:, None, None, None]
  e3 = lambda x: x[:, None, None]
  want = e4(ad) * r64['dW_expected'] + e4(bd) * r64['dW_log_prob']
  bound = e4(ad.abs()) * _bound(p, 'dW_expected') + e4(bd.abs()) * _bound(p, 'dW_log_prob')
  assert not torch.isnan(dW).any() and not torch.isnan(dl).any() and not torch.isnan(db).any()
  assert ((dW.double().cpu() - want).abs() <= bound).all()
  assert ((dl.double().cpu() - e3(ad) * r64['emission']).abs() <=
          e3(ad.abs()) * FACTOR * err['emission']).all()
  assert ((db.double().cpu() - e3(ad) * r64['blank_occ']).abs() <=
          e3(ad.abs()) * FACTOR * err['blank_occ']).all()
  # a second backward through the same graph recomputes: the same bits
  dW2, dl2, db2 = torch.autograd.grad(loss, [table, lv, bv])
  assert torch.equal(dW, dW2) and torch.equal(dl, dl2) and torch.equal(db, db2)


def test_bf16_weights_through_the_autograd_function(cuda):
  """dW is cast to W's dtype: for bf16 that rounding (2^-9 relative; the bound
  allows 2^-8, as test_gpu_expectation.py does) joins the bound."""
  p = _problem('p2_u100_t104_ws_bf16')
  r64 = p['r64']
  graph, W, d = _dev(p, cuda)
  W = W.requires_grad_(True)
  E, lp = lattices._AlignExpectFn.apply(W, d['lv'], d['bv'], d['nf'], d['lab'], d['nl'], graph)
  _check_values(p, E.detach(), lp.detach())
  (dW,) = torch.autograd.grad(E.sum(), [W])
  assert dW.dtype == torch.bfloat16
  want = r64['dW_expected']
  assert ((dW.double().cpu() - want).abs() <= _bound(p, 'dW_expected') + 2.0 ** -8 * want.abs()).all()


def _scatter_reference(p, g_lex, g_blank):
  """index_put_(accumulate=True) on the host in float64: the live frames and
  the positions up to num_labels of each utterance."""
  W, lab, ctx = p['W'], p['lab'].long(), p['ctx']
  B, T, C, R = W.shape
  U = lab.shape[-1]
  V = R - 1
  states = ctx.walk_states(torch.where((lab >= 1) & (lab <= V), lab, torch.zeros_like(lab)))
  safe = torch.where((lab >= 1) & (lab <= V), lab, torch.ones_like(lab))
  dW = torch.zeros([B, T, C, R], dtype=torch.float64)
  for b in range(B):
    nf, nl = int(p['nf'][b]), int(p['nl'][b])
    t = torch.arange(nf)[:, None]
    dW[b].index_put_((t.expand(nf, nl), states[b, :nl][None].expand(nf, nl),
                      safe[b, :nl][None].expand(nf, nl)), g_lex[b, :nf, :nl].double(),
                     accumulate=True)
    dW[b].index_put_((t.expand(nf, nl + 1), states[b, :nl + 1][None].expand(nf, nl + 1),
                      torch.zeros([nf, nl + 1], dtype=torch.long)),
                     g_blank[b, :nf, :nl + 1].double(), accumulate=True)
  return dW


@pytest.mark.parametrize('name', ['repeated_pair', 'trigram_v5_eps'])
def test_scatter_alone(cuda, name):
  """Random string gradients, NaN on the padding frames and past num_labels
  (not read): shared cells are summed (a chain of up to U / 2 positions in
  fp32 against float64: (chain length) x 2^-24 x the sum of magnitudes), the
  rest of dW is exactly zero, on poisoned memory, twice the same bits."""
  p = _problem(name)
  graph, W, d = _dev(p, cuda)
  B, T, U = p['lv'].shape
  g = torch.Generator().manual_seed(5)
  g_lex, g_blank = torch.randn([B, T, U], generator=g), torch.randn([B, T, U + 1], generator=g)
  want = _scatter_reference(p, g_lex, g_blank)
  mag = _scatter_reference(p, g_lex.abs(), g_blank.abs())
  if name == 'repeated_pair':  # most positions share a cell
    shared = (_scatter_reference(p, torch.ones_like(g_lex), torch.ones_like(g_blank)) > 1).sum()
    assert shared > 0.5 * (want != 0).sum()
  for b in range(B):
    nf, nl = int(p['nf'][b]), int(p['nl'][b])
    g_lex[b, nf:], g_blank[b, nf:] = torch.nan, torch.nan
    g_lex[b, :, nl:], g_blank[b, :, nl + 1:] = torch.nan, torch.nan
  with poisoned_buffers.poisoned(nat):
    dW = _scatter(graph, W, d, g_lex.to(cuda), g_blank.to(cuda))
  again = _scatter(graph, W, d, g_lex.to(cuda), g_blank.to(cuda))
  assert torch.equal(dW, again)
  dW = dW.double().cpu()
  assert not torch.isnan(dW).any()
  assert ((dW - want).abs() <= (U + 1) * 2.0 ** -24 * mag).all()
  assert (dW[want == 0] == 0).all()


@pytest.mark.parametrize('name', ['p4_u130_t50_lds', 'p4_u130_t51_ws', 'minus_inf'])
def test_poisoned_and_stale_buffers_determinism_and_the_value_only_call(cuda, name):
  """Every output and workspace byte is the call's own: the results on 0xFF
  memory, and on the memory a finished call on another problem of the same
  shape (other data, other padding rows) left behind, are bit-equal to a
  plain run; so are two plain runs; the value-only call gives the same
  expected and log_prob and needs no workspace."""
  p, q = _problem(name), _problem(name, '-other')
  graph, W, d = _dev(p, cuda)
  graph2, W2, d2 = _dev(q, cuda)
  if name != 'minus_inf':  # other padding rows
    d2['nf'] = torch.tensor([W.shape[1] - 7, 5, 0, W.shape[1]], dtype=torch.int32, device=cuda)
    d2['nl'] = torch.tensor([3, 5, 0, 40], dtype=torch.int32, device=cuda)

  def call(graph_, W_, d_):
    out = _expect(graph_, W_, d_)
    return out + (_scatter(graph_, W_, d_, out[4], out[5]),)

  plain = [x.clone() for x in call(graph, W, d)]
  again = call(graph, W, d)
  assert all(torch.equal(x, y) for x, y in zip(plain, again))
  with poisoned_buffers.poisoned(nat):
    got = call(graph, W, d)
    only = _expect(graph, W, d, want_post=False, want_cov=False)
  assert all(torch.equal(x, y) for x, y in zip(plain, got))
  assert only[2:] == (None, None, None, None)
  assert torch.equal(only[0], plain[0]) and torch.equal(only[1], plain[1])
  with poisoned_buffers.stale(nat) as s:
    s.record(call, graph2, W2, d2)
    got = s.replay(call, graph, W, d)
    assert all(torch.equal(x, y) for x, y in zip(plain, got))


def test_the_value_only_call_writes_nothing_but_its_two_outputs(cuda):
  """All four arrays NULL and no workspace, past the LDS rule: the call
  succeeds and expected / log_prob are the full call's bits."""
  p = _problem('p1_u20_t211_ws')
  graph, W, d = _dev(p, cuda)
  full = _expect(graph, W, d)
  B = W.shape[0]
  E = torch.full([B], 7.0, device=cuda)
  lp = torch.full([B], 7.0, device=cuda)
  pb = nat._tproblem(graph, W, d['lab'].shape[-1])
  nat._check(nat.lib().lt_table_align_expectation(
      ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(W), nat._ptr(d['lv']), nat._ptr(d['bv']),
      nat._ptr(d['nf']), nat._ptr(d['lab']), nat._ptr(d['nl']), nat._ptr(E), nat._ptr(lp), None,
      None, None, None, None, 0, nat._stream()), 'value-only call')
  assert torch.equal(E, full[0]) and torch.equal(lp, full[1])


@pytest.mark.parametrize('name,K,V,T,U', [('fld2_u12', 2, 4, 20, 12), ('fd_u256', 0, 8, 260, 256)])
def test_beyond_kernel_range_runs_the_restatement_on_the_device(cuda, name, K, V, T, U):
  """FrameLabelDependent(2) and U = 256 are past the kernels: the workspace
  query and both calls refuse (LT_EUNSUPPORTED) and
  RecognitionLattice.align_expectation answers with cpu.align_expectation on
  the tensors' own device, values and gradients within the same bounds."""
  rng = np.random.default_rng(zlib.crc32(name.encode()))
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  B = 4
  W = torch.tensor(rng.standard_normal((B, T, ctx.num_states(), V + 1)).astype(np.float32))
  nf = torch.tensor([T, T - 3, 1, 0], dtype=torch.int32)
  nl = torch.tensor([U if K == 0 else min(U, 2 * T), 5, 1, 0], dtype=torch.int32)
  lab = torch.tensor(rng.integers(1, V + 1, (B, U)).astype(np.int32))
  lv = torch.tensor(rng.standard_normal((B, T, U)).astype(np.float32))
  bv = torch.tensor(rng.standard_normal((B, T, U + 1)).astype(np.float32))
  r64, err = ref.yardstick(W, nf, lab, nl, ctx, lv, bv, K)
  fin = torch.isfinite(r64['log_prob'])
  assert fin.all()
  p = dict(name=name, r64=r64, err=err, fin=fin,
           post_bound=FACTOR * max(err['emission'], err['blank_occ']))
  table = W.to(cuda).requires_grad_(True)
  lat = ref.lattice(ctx, K, table)
  graph = lat._graph(cuda)
  dev = [x.to(cuda) for x in (nf, lab, nl)]
  assert not nat.table_align_expectation_supported(graph, table.detach(), dev[1])
  with pytest.raises(nat.LatticeLibraryError, match=r'\(-2\)'):
    nat.table_align_expectation(graph, table.detach(), lv.to(cuda), bv.to(cuda), *dev)
  with pytest.raises(nat.LatticeLibraryError, match=r'\(-2\)'):
    nat.table_string_scatter(graph, table.detach(), lv.to(cuda), bv.to(cuda), *dev)
  lvd, bvd = lv.to(cuda).requires_grad_(True), bv.to(cuda).requires_grad_(True)
  E, lp = lat.align_expectation(ref.frames((B,), T, cuda), dev[0], dev[1], dev[2], lvd, bvd)
  assert E.device.type == 'cuda' and lp.device.type == 'cuda'
  _check_values(p, E.detach(), lp.detach())
  dW, dl, db = torch.autograd.grad(E.sum(), [table, lvd, bvd])
  assert dW.device.type == 'cuda'
  assert _err(dW, r64['dW_expected']) <= _bound(p, 'dW_expected')
  assert _err(dl, r64['emission']) <= FACTOR * err['emission']
  assert _err(db, r64['blank_occ']) <= FACTOR * err['blank_occ']


def test_batch_dims_and_shape_errors_on_the_device(cuda):
  p = _problem('mixed_nf')
  graph, W, d = _dev(p, cuda)
  B, T, U = p['lv'].shape
  lat = ref.lattice(p['ctx'], 0, W.reshape(2, 4, *W.shape[1:]))
  fr = ref.frames((2, 4), T, cuda)
  shape = lambda x: x.reshape(2, 4, *x.shape[1:])
  E, lp = lat.align_expectation(fr, shape(d['nf']), shape(d['lab']), shape(d['nl']),
                                shape(d['lv']), shape(d['bv']))
  assert tuple(E.shape) == (2, 4) and tuple(lp.shape) == (2, 4) and not E.requires_grad
  full = _expect(graph, W, d)
  assert torch.equal(E.reshape(B), full[0]) and torch.equal(lp.reshape(B), full[1])
  E0, _ = lat.align_expectation(fr, shape(d['nf']), shape(d['lab']), shape(d['nl']),
                                shape(d['lv']))
  want = (full[2].double() * d['lv'].double()).sum((1, 2))
  np.testing.assert_allclose(E0.reshape(B).double().cpu().numpy(), want.cpu().numpy(), rtol=1e-4,
                             atol=1e-4)
  with pytest.raises(ValueError, match='lexical_values'):
    lat.align_expectation(fr, shape(d['nf']), shape(d['lab']), shape(d['nl']), d['lv'])
  with pytest.raises(ValueError, match='blank_values'):
    lat.align_expectation(fr, shape(d['nf']), shape(d['lab']), shape(d['nl']), shape(d['lv']),
                          shape(d['bv'])[..., :U])


def test_graph_capture_replays_match_eager(cuda):
  """One lt_table_align_expectation + lt_table_string_scatter pair (a single
  chain of two kernel nodes) captured into a graph and replayed on
  new weights, values and labels: the same bits as eager calls on them."""
  p = _problem('p2_u100_t104_ws')
  graph, W, d = _dev(p, cuda)
  B, T, U = p['lv'].shape
  C, R = W.shape[2:]
  pb = nat._tproblem(graph, W, U)
  nbytes = ctypes.c_size_t(0)
  nat._check(nat.lib().lt_table_align_expectation_workspace_bytes(
      ctypes.byref(graph.g), ctypes.byref(pb), ctypes.byref(nbytes)), 'query')
  assert nbytes.value > 0
  ws = torch.empty([nbytes.value], dtype=torch.uint8, device=cuda)
  W, lv, bv, lab = W.clone(), d['lv'].clone(), d['bv'].clone(), d['lab'].clone()
  E, lp = torch.empty([B], device=cuda), torch.empty([B], device=cuda)
  em, cl = torch.empty([B, T, U], device=cuda), torch.empty([B, T, U], device=cuda)
  bo, cb = torch.empty([B, T, U + 1], device=cuda), torch.empty([B, T, U + 1], device=cuda)
  dW = torch.empty([B, T, C, R], device=cuda)

  def call():
    nat._check(nat.lib().lt_table_align_expectation(
        ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(W), nat._ptr(lv), nat._ptr(bv),
        nat._ptr(d['nf']), nat._ptr(lab), nat._ptr(d['nl']), nat._ptr(E), nat._ptr(lp),
        nat._ptr(em), nat._ptr(bo), nat._ptr(cl), nat._ptr(cb), nat._ptr(ws), ws.numel(),
        nat._stream()), 'lt_table_align_expectation')
    nat._check(nat.lib().lt_table_string_scatter(
        ctypes.byref(graph.g), ctypes.byref(pb), nat._ptr(cl), nat._ptr(cb), nat._ptr(d['nf']),
        nat._ptr(lab), nat._ptr(d['nl']), nat._ptr(dW), nat._stream()), 'lt_table_string_scatter')

  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    call()  # eager on the side stream first, as torch's capture recipe does
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    call()
  first = None
  for seed in (2, 3):
    gen = torch.Generator().manual_seed(seed)
    W.copy_(torch.randn(W.shape, generator=gen))
    lv.copy_(torch.randn(lv.shape, generator=gen))
    bv.copy_(torch.randn(bv.shape, generator=gen))
    lab.copy_(torch.randint(1, R, lab.shape, generator=gen, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    d2 = dict(d, lv=lv, bv=bv, lab=lab)
    want = _expect(graph, W, d2)
    want_dW = _scatter(graph, W, d2, want[4], want[5])
    torch.cuda.synchronize()
    for x, y in zip((E, lp, em, bo, cl, cb, dW), want + (want_dW,)):
      assert torch.equal(x, y), seed
    if first is None:
      first = E.clone()
  assert not torch.equal(first, E)  # the replays did see the new inputs
