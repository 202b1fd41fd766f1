"""RecognitionLattice.align_expectation for long label strings on the GPU
(lt_table_align_expectation_long and lt_table_string_scatter_long,
lt_align_expect_long.hip; 256 <= U <= 1023) against the float64 reference of
tests/align_expect_ref.py: at the wave counts' boundaries with the mass and
the means crossing every wave boundary (T = U + 7), bf16, a table too large to
stage with epsilons, -inf arcs with NaN values under them, the pipeline's
block boundaries, the scatter alone, poisoned and stale memory, graph capture.

Bounds: test_gpu_align_expect.py's (_check_arrays, _bound, FACTOR): arrays and
the dense dW at most FACTOR x the float32 yardstick's error on that key;
expected and log_prob within the larger of the project's rtol = atol = 1e-4
and FACTOR x the yardstick's error on that key (a sum over about 1000 frames
in fp32). Every figure is printed before it is asserted (pytest -s).
"""
import zlib

import numpy as np
import pytest
import torch

import last_torch_amd as lt
from last_torch_amd import _native as nat
from last_torch_amd import cpu
import align_expect_ref as ref
import poisoned_buffers
from test_gpu_align_expect import FACTOR, _bound, _check_arrays, _err, _scatter_reference

pytestmark = pytest.mark.gpu

F = 16  # kXlF of lt_align_expect_long.hip: frames of a pipeline block
MINUS_INF_SALT = 'salt-0'  # picked on the CPU: utterances 0-2 stay aligned in the reference

CASES = [
    # name, V, C (random table) or None (bigram), U, dtype, epsilon, -inf, T - U. T = U + 7: the
    # only paths run near the diagonal, so mass and means cross every wave boundary
    ('u256', 4, None, 256, 'f32', False, False, 7),   # the first position of a second wave
    ('u511', 4, None, 511, 'f32', False, False, 7),
    ('u512', 4, None, 512, 'f32', False, False, 7),   # NW 2 -> 3
    ('u767', 4, None, 767, 'f32', False, False, 7),
    ('u768', 4, None, 768, 'f32', False, False, 7),   # NW 3 -> 4
    ('u1023', 4, None, 1023, 'f32', False, False, 7),
    ('bf16_u512', 4, None, 512, 'bf16', False, False, 7),
    ('table_c300_v28_u300_eps', 28, 300, 300, 'f32', True, False, 7),  # too large to stage in LDS
    ('minus_inf_u300', 4, None, 300, 'f32', False, True, 40),
    ('u300', 4, None, 300, 'f32', False, False, 7),   # the hygiene and capture tests'
]
_BY_NAME = {c[0]: c for c in CASES}
_PROBLEMS = {}


def _finish(name, ctx, W, nf, nl, lab, lv, bv, dt='f32'):
  r64, err = ref.yardstick(W, nf, lab, nl, ctx, lv, bv)
  return dict(name=name, ctx=ctx, W=W, nf=nf, nl=nl, lab=lab, lv=lv, bv=bv, dt=dt, r64=r64, err=err,
              fin=torch.isfinite(r64['log_prob']),
              post_bound=FACTOR * max(err['emission'], err['blank_occ']))


def _problem(name, variant=''):
  """test_gpu_align_post_long._problem's recipe with values: four utterances
  (full length, a little shorter, empty, three frames with one label too
  many), N(0, 1) weights and values of both kinds, seeded from the name;
  computed once, changed by nothing."""
  key = name + variant
  if key not in _PROBLEMS:
    _, V, C, U, dt, eps, minf, slack = _BY_NAME[name]
    T = U + slack
    rng = np.random.default_rng(zlib.crc32((key + (MINUS_INF_SALT if minf else '')).encode()))
    if C is None:
      ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
    else:
      ctx = lt.contexts.NextStateTable(torch.tensor(rng.integers(0, C, (C, V)).astype(np.int32)))
    W = rng.standard_normal((4, T, ctx.shape()[0], V + 1)).astype(np.float32)
    if minf:
      W[rng.random(W.shape) < 0.05] = -np.inf
    W = torch.tensor(W)
    if dt == 'bf16':
      W = W.bfloat16().float()
    nf = torch.tensor([T, T, 0, 3], dtype=torch.int32)
    nl = torch.tensor([U, U - 2, 0, 4], dtype=torch.int32)
    lab = torch.tensor(rng.integers(0 if eps else 1, V + 1, (4, U)).astype(np.int32))
    lv = torch.tensor(rng.standard_normal((4, T, U)).astype(np.float32))
    bv = torch.tensor(rng.standard_normal((4, T, U + 1)).astype(np.float32))
    if minf:  # NaN under every -inf arc: never read into the arithmetic
      blank, lex = cpu.string_weights(W, lab.long(), ctx)
      lv[~torch.isfinite(lex)] = torch.nan
      bv[~torch.isfinite(blank)] = torch.nan
    p = _finish(name, ctx, W, nf, nl, lab, lv, bv, dt)
    # the reference alone leaves only the short utterance unaligned
    assert p['fin'].tolist() == [True, True, True, False] and p['r64']['log_prob'][2] == 0
    _PROBLEMS[key] = p
  return _PROBLEMS[key]


def _dev(p, cuda):
  W = p['W'].to(cuda)
  graph = ref.lattice(p['ctx'], 0, W)._graph(cuda)
  if p['dt'] == 'bf16':
    W = W.bfloat16()
  return graph, W.contiguous(), {k: p[k].to(cuda) for k in ('nf', 'lab', 'nl', 'lv', 'bv')}


def _expect(graph, W, d, **kw):
  return nat.table_align_expectation_long(graph, W, d['lv'], d['bv'], d['nf'], d['lab'], d['nl'],
                                          **kw)


def _scatter(graph, W, d, g_lex, g_blank):
  return nat.table_string_scatter_long(graph, W, g_lex, g_blank, d['nf'], d['lab'], d['nl'])


def _check_values(p, E, lp):
  E, lp = E.double().cpu(), lp.double().cpu()
  fin, r64, err = p['fin'], p['r64'], p['err']
  assert torch.isfinite(E).all() and not torch.isnan(lp).any()
  assert torch.equal(torch.isfinite(lp), fin) and (lp[~fin] == -torch.inf).all()
  assert (E[~fin] == 0).all()
  print(f"\n{p['name']}: expected {_err(E, r64['expected']):.3g} / {err['expected']:.3g} log_prob "
        f"{_err(lp[fin], r64['log_prob'][fin]):.3g} / {err['log_prob']:.3g}", end='')
  for got, key in ((E[fin], 'expected'), (lp[fin], 'log_prob')):
    want = r64[key][fin]
    assert ((got - want).abs() <= torch.clamp(1e-4 + 1e-4 * want.abs(), min=FACTOR * err[key])).all()


def _check_call_and_autograd(p, cuda):
  """Both ABI calls through the bindings, then the public method with autograd."""
  r64, err = p['r64'], p['err']
  graph, W, d = _dev(p, cuda)
  assert nat.table_align_expectation_long_supported(graph, W, d['lab'])
  assert not nat.table_align_expectation_supported(graph, W, d['lab'])
  E, lp, em, bo, cl, cb = _expect(graph, W, d)
  _check_values(p, E, lp)
  _check_arrays(p, em, bo, cl, cb)
  if p['dt'] == 'bf16':  # TableWeightFn hands out fp32: the bf16 kernel through the bindings
    dwe, dwl = _scatter(graph, W, d, cl, cb), _scatter(graph, W, d, em, bo)
  else:
    table = p['W'].to(cuda).requires_grad_(True)
    B, T = W.shape[:2]
    lat = ref.lattice(p['ctx'], 0, table)
    E2, lp2 = lat.align_expectation(ref.frames((B,), T, cuda), d['nf'], d['lab'], d['nl'], d['lv'],
                                    d['bv'])
    assert torch.equal(E2, E) and torch.equal(lp2, lp) and E2.requires_grad and lp2.requires_grad
    (dwe,) = torch.autograd.grad(E2.sum(), [table], retain_graph=True)
    (dwl,) = torch.autograd.grad(torch.where(torch.isfinite(lp2), lp2, 0).sum(), [table])
  k_e, k_l = _err(dwe, r64['dW_expected']), _err(dwl, r64['dW_log_prob'])
  print(f" | dW_expected {k_e:.3g} / {err['dW_expected']:.3g} | dW_log_prob {k_l:.3g} / "
        f"{err['dW_log_prob']:.3g}", end='')
  assert not torch.isnan(dwe).any() and not torch.isnan(dwl).any()
  assert k_e <= _bound(p, 'dW_expected') and k_l <= _bound(p, 'dW_log_prob')
  live = (torch.arange(W.shape[1])[None] < p['nf'][:, None]) & p['fin'][:, None]
  assert not dwe.cpu()[~live].any() and not dwl.cpu()[~live].any()


@pytest.mark.parametrize('name', [c[0] for c in CASES[:-1]])
def test_long_align_expectation_matches_reference(cuda, name):
  _check_call_and_autograd(_problem(name), cuda)


def test_pipeline_block_boundaries(cuda):
  """num_frames 1, 2, F-1, F, F+1, 2F, 2F+1, 4F+3 in one batch at max_labels =
  300 (two waves a direction): odd and even midpoints, phases shorter than one
  block, blocks shorter than the skew, drain and refill with no full block."""
  V, U = 4, 300
  nf = torch.tensor([1, 2, F - 1, F, F + 1, 2 * F, 2 * F + 1, 4 * F + 3], dtype=torch.int32)
  nl = torch.tensor([1, 2, F - 1, F - 3, F + 1, 2 * F, 2 * F - 5, 4 * F + 3], dtype=torch.int32)
  B, T = len(nf), int(nf.max())
  rng = np.random.default_rng(4 * F + 3)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=1)
  W = torch.tensor(rng.standard_normal((B, T, ctx.num_states(), V + 1)).astype(np.float32))
  lab = torch.tensor(rng.integers(1, V + 1, (B, U)).astype(np.int32))
  lv = torch.tensor(rng.standard_normal((B, T, U)).astype(np.float32))
  bv = torch.tensor(rng.standard_normal((B, T, U + 1)).astype(np.float32))
  p = _finish('block_boundaries', ctx, W, nf, nl, lab, lv, bv)
  assert p['fin'].all()
  _check_call_and_autograd(p, cuda)


@pytest.mark.parametrize('V,n,eps', [(4, 1, False), (5, 2, True)])
def test_scatter_alone(cuda, V, n, eps):
  """Random string gradients at U = 300, NaN on the padding frames and past
  num_labels (not read). At V = 4 every cell is shared by dozens of positions:
  a chain of up to U + 1 entries in fp32 against float64 is (chain length) x
  2^-24 x the sum of magnitudes; the rest of dW is exactly zero, on poisoned
  memory, twice the same bits. T = 70: two workgroups of rows an utterance."""
  B, T, U = 3, 70, 300
  rng = np.random.default_rng(300 + V)
  ctx = lt.contexts.FullNGram(vocab_size=V, context_size=n)
  p = dict(ctx=ctx, W=torch.zeros([B, T, ctx.num_states(), V + 1]),
           lab=torch.tensor(rng.integers(0 if eps else 1, V + 1, (B, U)).astype(np.int32)),
           nf=torch.tensor([T, 65, 0], dtype=torch.int32),
           nl=torch.tensor([U, 257, 0], dtype=torch.int32))
  graph = ref.lattice(ctx, 0, p['W'].to(cuda))._graph(cuda)
  d = {k: p[k].to(cuda) for k in ('nf', 'lab', 'nl')}
  g = torch.Generator().manual_seed(5)
  g_lex, g_blank = torch.randn([B, T, U], generator=g), torch.randn([B, T, U + 1], generator=g)
  want = _scatter_reference(p, g_lex, g_blank)
  mag = _scatter_reference(p, g_lex.abs(), g_blank.abs())
  count = _scatter_reference(p, torch.ones_like(g_lex), torch.ones_like(g_blank))
  if not eps:
    assert count[0, 0].max() >= 50 and (count[0, 0] >= 12).sum() >= 10  # dozens of positions a cell
  for b in range(B):
    nf, nl = int(p['nf'][b]), int(p['nl'][b])
    g_lex[b, nf:], g_blank[b, nf:] = torch.nan, torch.nan
    g_lex[b, :, nl:], g_blank[b, :, nl + 1:] = torch.nan, torch.nan
  Wd = p['W'].to(cuda)
  with poisoned_buffers.poisoned(nat):
    dW = _scatter(graph, Wd, d, g_lex.to(cuda), g_blank.to(cuda))
  again = _scatter(graph, Wd, d, g_lex.to(cuda), g_blank.to(cuda))
  assert torch.equal(dW, again)
  dW = dW.double().cpu()
  assert not torch.isnan(dW).any()
  print(f'\nscatter V={V}: max chain {int(count.max())}, error {float((dW - want).abs().max()):.3g}')
  assert ((dW - want).abs() <= count * 2.0 ** -24 * mag).all()
  assert (dW[want == 0] == 0).all()


def test_long_poisoned_and_stale_buffers_determinism_and_the_value_only_call(cuda):
  """Every output and workspace byte is the call's own: the results on 0xFF
  memory, and on the memory a finished call on another problem of the same
  shape left behind, are bit-equal to a plain run, for both calls; so are two
  plain runs; the value-only call allocates and writes nothing but expected
  and log_prob, and they are the full call's bits."""
  p, q = _problem('u300'), _problem('u300', '-other')
  graph, W, d = _dev(p, cuda)
  graph2, W2, d2 = _dev(q, cuda)
  T = W.shape[1]
  d2['nf'] = torch.tensor([T - 7, 5, 0, T], dtype=torch.int32, device=cuda)  # other padding rows
  d2['nl'] = torch.tensor([3, 5, 0, 290], dtype=torch.int32, device=cuda)

  def call(graph_, W_, d_):
    out = _expect(graph_, W_, d_)
    return out + (_scatter(graph_, W_, d_, out[4], out[5]),)

  plain = [x.clone() for x in call(graph, W, d)]
  again = call(graph, W, d)
  assert all(torch.equal(x, y) for x, y in zip(plain, again))
  with poisoned_buffers.poisoned(nat):
    got = call(graph, W, d)
  assert all(torch.equal(x, y) for x, y in zip(plain, got))
  with poisoned_buffers.stale(nat) as s:
    only = s.record(_expect, graph, W, d, want_post=False, want_cov=False)
    assert len(s.tensors) == 2  # no workspace, no array
  assert only[2:] == (None, None, None, None)
  assert torch.equal(only[0], plain[0]) and torch.equal(only[1], plain[1])
  with poisoned_buffers.stale(nat) as s:
    s.record(call, graph2, W2, d2)
    got = s.replay(call, graph, W, d)
    assert all(torch.equal(x, y) for x, y in zip(plain, got))


def test_graph_capture_of_forward_and_backward_through_the_public_method(cuda):
  """One captured graph holds align_expectation and its backward (the long
  kernel, the long scatter and the torch ops between them) at U = 300;
  replayed on new weights it gives the eager call's bits, every time."""
  p, q = _problem('u300'), _problem('u300', '-other')
  _, _, d = _dev(p, cuda)
  B, T = p['W'].shape[:2]
  frames = ref.frames((B,), T, cuda)

  def run(lat, table):
    E, lp = lat.align_expectation(frames, d['nf'], d['lab'], d['nl'], d['lv'], d['bv'])
    loss = (E + 0.5 * torch.where(torch.isfinite(lp), lp, 0)).sum()
    return E, lp, torch.autograd.grad(loss, [table])[0]

  def eager(W):
    table = W.to(cuda).requires_grad_(True)
    return run(ref.lattice(p['ctx'], 0, table), table)

  table = p['W'].to(cuda).requires_grad_(True)
  lat = ref.lattice(p['ctx'], 0, table)  # reads `table` at every call
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    run(lat, table)  # eager on the side stream first, as torch's capture recipe does
  torch.cuda.current_stream().wait_stream(s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = run(lat, table)
  first = None
  for W2 in (q['W'], p['W'], q['W']):
    with torch.no_grad():
      table.copy_(W2)
    g.replay()
    torch.cuda.synchronize()
    want = eager(W2)
    torch.cuda.synchronize()
    for x, y in zip(out, want):
      assert torch.equal(x, y)
    first = out[0].clone() if first is None else first
  assert not torch.equal(first, eager(p['W'])[0])  # the replays did see the new weights
