"""GRADIENT COMPOSITION PIN -- TF primitive gradients ASSUMED and listed.

The sibling of make_reference_facade.py for the BACKWARD passes.  The same bodies of the reference's TensorFlow methods
(cut out of the files by ``ast``; ``process`` / ``filter_param_regressor`` of the eight filter classes and ``LevelFilter``,
``Filter.get_mask`` and the statement filters.py:88, util.py's lrelu / rgb2lum / tanh01 / tanh_range / lerp, ``pdf_sample``
and agent.py:100-123, 208-252) are EXECUTED in the build container with a torch float64 stand-in as ``tf`` and autograd
switched on; what is stored is autograd's gradient of ``sum(y * dy)`` through the reference's own text.

TensorFlow is not installed, so every primitive's gradient is the stand-in's.  The TF-1 conventions are written here as
explicit ``torch.autograd.Function``s (never borrowed from a torch default), and each is named in the fixture's op list:

  maximum(x, c) / minimum(x, c), c a Python scalar   the gradient goes to x where x >= c / x <= c (TF _MaximumMinimumGrad);
      with two tensor operands (agent.py:234 only) nothing may require a gradient: torch would split ties 50 / 50
  clip_by_value(x, lo, hi)                             the composition of the two: passes on lo <= x <= hi, both inclusive
  abs                                                  sign(x), 0 at 0 (so util.lrelu' (0) = 0.5 (1 + leak) = 0.6)
  image.rgb_to_hsv / hsv_to_rgb                        hsv_grad_mode 0: the NumPy facade's functions on detached values, a
      constant (TF-1 registers both ops as not differentiable)
  pow, exp, log, cos, tanh, sigmoid, softmax, sums, cumsum, reshape, concat, slicing: torch's

What this pins: that the build's hand-derived backward code (oracle/filters_np.py, tests/_agent_glue_ref.py, the HIP
kernels) COMPOSES those primitive gradients the way back-propagation through the reference's statements does -- which
clip feeds which knot, that Gamma's floor and Contrast's luminance clamp block the gradient on the side TF blocks it, the
cross terms of the white-balance normalisation and of the entropy, the masks' six raw parameters.  What it cannot pin:
the primitives' gradients themselves.  A stand-in library pins no primitive.

A SECOND variant (key prefix ``hsv1_``) makes the two HSV ops differentiable, for the repository's analytic mode
(``hsv_grad_mode = 1``): the same published TF per-pixel formulas the NumPy facade uses outside [0, 1], written in
differentiable torch ops HERE.  That variant pins composition against THE BUILD'S STATEMENT of TF's formula, nothing more;
it comes with a boolean ``smooth`` mask (false where two channels tie, rng == 0, v == 0, v == 0.5 or a channel is >= 1).

Two mechanical rewrites of the cut-out bodies (and one name binding) were needed to run them under autograd; each is
recorded in the fixture under ``rewrites``.  The committed fixture holds inputs, cotangents, gradients, the stand-in's op
list, the rewrites and the sha256 of each source file -- data only.  tests/test_reference_grad_facade.py holds the CPU
oracles and (gpu) the HIP backward kernels against it.

  python tests/golden/make_reference_grad_facade.py        # rewrites tests/golden/reference_grad_facade.npz
"""
import ast
import contextlib
import copy
import math
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_reference_facade import FILTERS, HERE, REF, TfFacade, cut_span, methods_of, no_prints, sha256  # noqa: E402

T64 = torch.float64

REWRITES = [
    'np.array -> float64 tensor: the bodies get an `np` shim whose `array` returns a torch float64 tensor (the (0, 1, 1) '
    'mask of ImprovedWhiteBalanceFilter.filter_param_regressor multiplies a tensor); everything else forwards to NumPy',
    'AugAssign -> Assign: every `target <op>= value` of the cut bodies becomes `target = target <op> value` '
    '(ast.NodeTransformer; value-identical): filters.py:232 and :140 write in place into tensors autograd has saved',
    'builtin abs -> the stand-in: util.py:229 calls Python\'s abs(x); the name is bound to the stand-in\'s abs so that '
    'abs\'(0) = 0 is the listed convention and not torch\'s',
]


class _MaxConst(torch.autograd.Function):
  """tf.maximum(x, c): the gradient goes to x where x >= c."""

  @staticmethod
  def forward(ctx, x, c):
    ctx.save_for_backward(x >= c)
    return torch.clamp_min(x.detach(), c)

  @staticmethod
  def backward(ctx, g):
    return g * ctx.saved_tensors[0].to(g.dtype), None


class _MinConst(torch.autograd.Function):
  """tf.minimum(x, c): the gradient goes to x where x <= c."""

  @staticmethod
  def forward(ctx, x, c):
    ctx.save_for_backward(x <= c)
    return torch.clamp_max(x.detach(), c)

  @staticmethod
  def backward(ctx, g):
    return g * ctx.saved_tensors[0].to(g.dtype), None


class _Abs(torch.autograd.Function):
  """tf.abs: sign(x), 0 at 0."""

  @staticmethod
  def forward(ctx, x):
    ctx.save_for_backward(x)
    return x.detach().abs()

  @staticmethod
  def backward(ctx, g):
    x, = ctx.saved_tensors
    return g * ((x > 0).to(g.dtype) - (x < 0).to(g.dtype))


class TorchTf:
  """torch float64 stand-ins, autograd on, for the TensorFlow-1 primitives the cut-out bodies use; every call is
  recorded.  ``hsv_grad_mode`` 0: HSV ops are constants; 1: differentiable TF formulas."""

  int32, float32 = torch.int32, T64

  def __init__(self, hsv_grad_mode=0):
    self.used = set()
    facade = self
    np_facade = TfFacade()

    class image:  # tf.image

      @staticmethod
      def rgb_to_hsv(x):
        if hsv_grad_mode == 0:
          facade.used.add('image.rgb_to_hsv [NumPy facade on detached values: a constant (TF-1: not differentiable)]')
          return torch.from_numpy(np_facade.image.rgb_to_hsv(x.detach().numpy()))
        facade.used.add('image.rgb_to_hsv [TF formula in differentiable torch ops: hsv_grad_mode 1]')
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        v = x.max(dim=-1).values
        rng_ = v - x.min(dim=-1).values
        one = torch.ones_like(v)
        sat = torch.where(v > 0, rng_ / torch.where(v > 0, v, one), torch.zeros_like(v))
        norm = 1.0 / (6.0 * torch.where(rng_ > 0, rng_, one))
        hue = torch.where(r == v, norm * (g - b), torch.where(g == v, norm * (b - r) + 2.0 / 6.0, norm * (r - g) + 4.0 / 6.0))
        hue = torch.where(rng_ > 0, hue, torch.zeros_like(hue))
        hue = torch.where(hue < 0, hue + 1.0, hue)
        return torch.stack([hue, sat, v], dim=-1)

      @staticmethod
      def hsv_to_rgb(x):
        if hsv_grad_mode == 0:
          facade.used.add('image.hsv_to_rgb [NumPy facade on detached values: a constant (TF-1: not differentiable)]')
          return torch.from_numpy(np_facade.image.hsv_to_rgb(x.detach().numpy()))
        facade.used.add('image.hsv_to_rgb [TF formula in differentiable torch ops: hsv_grad_mode 1]')
        hh, ss, vv = x[..., 0], x[..., 1], x[..., 2]
        dh = hh * 6.0
        clip01 = lambda t: _MinConst.apply(_MaxConst.apply(t, 0.0), 1.0)
        dr = clip01(_Abs.apply(dh - 3.0) - 1.0)
        dg = clip01(2.0 - _Abs.apply(dh - 2.0))
        db = clip01(2.0 - _Abs.apply(dh - 4.0))
        oms = 1.0 - ss
        return torch.stack([(oms + ss * dr) * vv, (oms + ss * dg) * vv, (oms + ss * db) * vv], dim=-1)

    class nn:  # tf.nn

      @staticmethod
      def softmax(x):
        facade.used.add('nn.softmax')
        return torch.softmax(x, dim=-1)

    self.image, self.nn = image, nn

  def _u(self, name):
    self.used.add(name)

  def maximum(self, x, y):
    if isinstance(y, (int, float)):
      self._u('maximum [scalar: gradient to x where x >= c]')
      return _MaxConst.apply(x, float(y))
    self._u('maximum [two tensors, no gradient]')
    assert not x.requires_grad and not y.requires_grad
    return torch.maximum(x, y)

  def minimum(self, x, y):
    assert isinstance(y, (int, float)), 'tf.minimum of two tensors: not in the cut bodies'
    self._u('minimum [scalar: gradient to x where x <= c]')
    return _MinConst.apply(x, float(y))

  def clip_by_value(self, x, lo, hi):
    self._u('clip_by_value [minimum(maximum(x, lo), hi): passes on lo <= x <= hi]')
    return _MinConst.apply(_MaxConst.apply(x, float(lo)), float(hi))

  def abs(self, x):
    self._u('abs [sign(x), 0 at 0]')
    return _Abs.apply(x)

  def exp(self, x): self._u('exp'); return torch.exp(x)
  def log(self, x): self._u('log'); return torch.log(x)
  def pow(self, x, y): self._u('pow'); return torch.pow(x, y)
  def cos(self, x): self._u('cos'); return torch.cos(x)
  def tanh(self, x): self._u('tanh'); return torch.tanh(x)
  def sigmoid(self, x): self._u('sigmoid'); return torch.sigmoid(x)
  def reshape(self, x, shape): self._u('reshape'); return torch.reshape(x, tuple(shape))
  def concat(self, values, axis): self._u('concat'); return torch.cat(list(values), dim=axis)
  def less(self, x, y): self._u('less'); return torch.lt(x, y)
  def cast(self, x, dtype): self._u('cast'); return x.to(dtype)
  def argmax(self, x, axis): self._u('argmax'); return torch.argmax(x, dim=axis)
  def constant(self, x): self._u('constant'); return torch.as_tensor(np.asarray(x), dtype=T64)

  def one_hot(self, ids, depth, dtype):
    self._u('one_hot')  # tf.one_hot: an index outside [0, depth) gives an all-zero row
    return (ids[:, None] == torch.arange(depth)[None, :]).to(dtype)

  def reduce_sum(self, x, axis=None, keep_dims=False):
    self._u('reduce_sum')
    return torch.sum(x) if axis is None else torch.sum(x, dim=axis, keepdim=keep_dims)

  def reduce_mean(self, x, axis=None, keep_dims=False):
    self._u('reduce_mean')
    return torch.mean(x) if axis is None else torch.mean(x, dim=axis, keepdim=keep_dims)

  def cumsum(self, x, axis, exclusive=False):
    self._u('cumsum')
    c = torch.cumsum(x, dim=axis)
    if exclusive:  # a SHIFTED inclusive scan
      c = torch.cat([torch.zeros_like(c.narrow(axis, 0, 1)), c.narrow(axis, 0, c.shape[axis] - 1)], dim=axis)
    return c

  @staticmethod
  def variable_scope(name):
    return contextlib.nullcontext()

  @staticmethod
  def name_scope(name=None):
    return contextlib.nullcontext()


class NpFacade(TfFacade):
  """The forward sibling's NumPy facade plus the two calls of Filter.get_mask (the forward cross-check of case C)."""

  def constant(self, x): self._u('constant'); return np.asarray(x, dtype=np.float64)

  @staticmethod
  def name_scope(name=None):
    return contextlib.nullcontext()


class NpShim:
  """``np`` as the bodies see it: ``array`` gives a float64 tensor, the rest is NumPy."""

  @staticmethod
  def array(obj, dtype=None):
    return torch.as_tensor(np.array(obj, dtype=np.float64), dtype=T64)

  def __getattr__(self, name):
    return getattr(np, name)


class NoAugAssign(ast.NodeTransformer):

  def visit_AugAssign(self, node):
    load = copy.deepcopy(node.target)
    for sub in ast.walk(load):
      if hasattr(sub, 'ctx'):
        sub.ctx = ast.Load()
    load.ctx = ast.Load()
    return ast.copy_location(ast.Assign(targets=[node.target], value=ast.BinOp(left=load, op=node.op, right=node.value),
                                        type_comment=None), node)


def compile_for(tree, name, rewrite):
  tree = copy.deepcopy(tree)
  if rewrite:
    tree = NoAugAssign().visit(tree)
  ast.fix_missing_locations(tree)
  return compile(tree, name, 'exec')


def namespaces(trees):
  """(torch hsv 0, torch hsv 1, NumPy facade) namespaces with every cut tree executed in them."""
  out = []
  for tf, rewrite in ((TorchTf(0), True), (TorchTf(1), True), (NpFacade(), False)):
    ns = {'tf': tf, 'math': math, 'print': lambda *a, **k: None}
    if rewrite:
      ns.update(np=NpShim(), abs=tf.abs)
    else:
      ns.update(np=np)
    for name, tree in trees:
      exec(compile_for(tree, name, rewrite), ns)
    out.append(ns)
  return out


def leaf(a):
  return torch.tensor(np.asarray(a, dtype=np.float64), dtype=T64, requires_grad=True)


def npy(t):
  return t.detach().numpy().copy()


def main():
  rng = np.random.default_rng(20261019)
  fwd = np.load(os.path.join(HERE, 'reference_facade.npz'))
  out, prov = {}, []

  u_path, f_path = os.path.join(REF, 'util.py'), os.path.join(REF, 'filters.py')
  p_path, a_path = os.path.join(REF, 'pdf_sample_layer.py'), os.path.join(REF, 'agent.py')
  for p in (u_path, f_path, p_path, a_path):
    prov.append((os.path.basename(p), sha256(p)))
  assert ['%s sha256=%s' % p for p in prov] == [str(s) for s in fwd['provenance']], 'reference_facade.npz was cut from another text'

  trees = [('<reference util.%s>' % n, cut_span(u_path, n)) for n in ('lrelu', 'rgb2lum', 'tanh01', 'tanh_range', 'lerp')]
  ftree = ast.parse(open(f_path).read(), filename=f_path)
  body = []
  for cls, _p in FILTERS:
    body += methods_of(ftree, cls, ['filter_param_regressor', 'process'])
  body += methods_of(ftree, 'Filter', ['get_mask'])
  trees.append(('<reference filters.py methods>', ast.Module(body=body, type_ignores=[])))
  ptree = ast.parse(open(p_path).read(), filename=p_path)
  trees.append(('<reference pdf_sample>', ast.Module(
      body=[next(nd for nd in ptree.body if isinstance(nd, ast.FunctionDef) and nd.name == 'pdf_sample')], type_ignores=[])))
  ns0, ns1, nsn = namespaces(trees)
  for ns in (ns0, ns1, nsn):
    ns.update(STATE_REWARD_DIM=0, STATE_STOPPED_DIM=1, STATE_STEP_DIM=2, STATE_DROPOUT_BEGIN=3)  # util.py (checked by the sibling)

  # filters.py:88, the one statement of Filter.apply that blends the processed image in
  apply_fn = next(fn for fn in next(n for n in ftree.body if isinstance(n, ast.ClassDef) and n.name == 'Filter').body
                  if isinstance(fn, ast.FunctionDef) and fn.name == 'apply')
  line88 = [s for s in apply_fn.body if s.lineno == 88]
  assert len(line88) == 1 and ast.unparse(line88[0]).replace(' ', '') == \
      'low_res_output=lerp(img,self.process(img,filter_parameters),self.mask)', ast.unparse(line88[0])
  line88 = compile_for(ast.Module(body=line88, type_ignores=[]), '<reference filters.py:88>', True)

  # ---- agent.py:100-123, 208-252 (case E below; its last statement, the penalty, also closes cases A and B) ---------
  atree = ast.parse(open(a_path).read(), filename=a_path)
  gen = next(nd for nd in atree.body if isinstance(nd, ast.FunctionDef) and nd.name == 'agent_generator')

  def statements(node, lo, hi, found):
    """The simple statements of lines lo..hi that run unconditionally (``with`` bodies yes, ``if`` / ``for`` / ``def`` no)."""
    for s in node.body:
      if isinstance(s, ast.With):
        statements(s, lo, hi, found)
      elif not isinstance(s, (ast.If, ast.For, ast.FunctionDef)) and lo <= s.lineno <= hi:
        found.append(s)
    return found

  sel = no_prints(statements(gen, 100, 123, []))
  assert ast.unparse(sel[0]).startswith('pdf = tf.nn.softmax(pdf) + 1e-37') and ast.unparse(sel[-1]).startswith('surrogate = ')
  upd = [s for s in no_prints(statements(gen, 208, 252, []))
         if not isinstance(s, ast.Assert) and 'regular_filter_start = 0' != ast.unparse(s)]
  assert ast.unparse(upd[0]).startswith('new_states = [None') and ast.unparse(upd[-1]).startswith('penalty = ')
  agent_code = compile_for(ast.Module(body=sel + upd, type_ignores=[]), '<reference agent.py:100-123, 208-252>', True)
  agent_code_np = compile_for(ast.Module(body=sel + upd, type_ignores=[]), '<reference agent.py:100-123, 208-252>', False)

  pen_code = compile_for(ast.Module(body=[upd[-1]], type_ignores=[]), '<reference agent.py:249-252>', True)

  def make_self(L, masking=False):
    cfg = types.SimpleNamespace(exposure_range=3.5, gamma_range=3, curve_steps=L, color_curve_range=(0.90, 1.10),
                                tone_curve_range=(0.5, 2), masking=masking, maximum_sharpness=1, minimum_strength=0.3)
    return types.SimpleNamespace(cfg=cfg, channels=3, curve_steps=L, use_masking=lambda: masking,
                                 get_num_mask_parameters=lambda: 6)

  def run_filter(ns, cls, L, x, features, dy, raw_mask=None, dpen=None):
    """params = regressor(features), y = process(x, params) [or filters.py:88 with the mask]; gradients of sum(y dy)
    [+ sum_n dpen_n penalty_n, the penalty statement agent.py:249-252 on net = y with its three other terms 0]."""
    self_ = make_self(L, masking=raw_mask is not None)
    xt, ft = leaf(x), leaf(features)
    params = ns['%s__filter_param_regressor' % cls](self_, ft)
    leaves = [xt, params, ft]
    if raw_mask is None:
      y = ns['%s__process' % cls](self_, xt, params)
    else:
      mt = leaf(raw_mask)
      leaves.append(mt)
      self_.process = lambda img, p: ns['%s__process' % cls](self_, img, p)
      self_.mask = ns['Filter__get_mask'](self_, xt, mt)
      env = dict(ns, self=self_, img=xt, filter_parameters=params)
      exec(line88, env)
      y = env['low_res_output']
    loss = (y * torch.from_numpy(dy)).sum()
    if dpen is not None:
      env = dict(ns, net=y, entropy_penalty=0.0, usage_penalty=0.0, early_stop_penalty=0.0,
                 cfg=types.SimpleNamespace(filter_usage_penalty=1.0))
      exec(pen_code, env)
      loss = loss + (env['penalty'][:, 0] * torch.from_numpy(dpen)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    res = dict(y=npy(y), params=npy(params), dx=npy(grads[0]), dparams=npy(grads[1]).reshape(x.shape[0], -1),
               dfeatures=npy(grads[2]))
    if raw_mask is not None:
      res['dmask_params'] = npy(grads[3])
    return res

  def numpy_y(cls, L, x, features, raw_mask=None):
    self_ = make_self(L, masking=raw_mask is not None)
    params = nsn['%s__filter_param_regressor' % cls](self_, features)
    y = nsn['%s__process' % cls](self_, x, params)
    if raw_mask is not None:
      y = nsn['lerp'](x, y, nsn['Filter__get_mask'](self_, x, raw_mask))
    return np.asarray(y)

  pen_is_plain = []

  def keep_pen(prefix, r):
    """Stores the gradients with the penalty in the loss -- or, where no output exceeds 1 by more than float64 rounding and
    they are the plain ones to 1e-13 (Tone, Color, SaturationPlus, Level), only the prefix in ``pen_is_plain``."""
    same = lambda a, b: np.abs(a - b).max() <= 1e-13 * (1.0 + np.abs(b).max())
    if r['y'].max() <= 1.0 + 1e-13 and same(r['dx'], out[prefix + '_dx']) and same(r['dparams'], out[prefix + '_dparams']):
      pen_is_plain.append(prefix)
    else:
      out[prefix + '_pen_dx'], out[prefix + '_pen_dparams'] = r['dx'], r['dparams']

  x = fwd['x']
  n, h, w, _ = x.shape
  dy = rng.standard_normal(x.shape)
  out['dy'] = dy
  dpen = (rng.standard_normal(n) * 50.0).astype(np.float32).astype(np.float64)  # d loss / d penalty, exact in fp32
  out['dpen'] = dpen

  # ---- A: the nine filters at curve_steps = 8, on the forward fixture's x and features ---------------------------------
  for cls, _p in FILTERS:
    f = fwd[cls + '_features']
    r = run_filter(ns0, cls, 8, x, f, dy)
    assert np.abs(r['y'] - fwd[cls + '_y']).max() <= 1e-13 and np.abs(r['params'] - fwd[cls + '_params']).max() <= 1e-13, cls
    for k in ('dx', 'dparams', 'dfeatures'):
      out['A_%s_%s' % (cls, k)] = r[k]
    r = run_filter(ns0, cls, 8, x, f, dy, dpen=dpen)  # the same with the over-exposure penalty of y in the loss
    keep_pen('A_%s' % cls, r)

  # ---- A2: Contrast again with a live parameter in image 0 (A's is tanh(0) = 0, which switches the filter off on exactly
  # the image that holds the lum = 1 tie: the luminance clamp's gradient rule would not show) ------------------------------
  f = fwd['ContrastFilter_features'].copy()
  f[0] = 0.75
  r = run_filter(ns0, 'ContrastFilter', 8, x, f, dy)
  assert np.abs(r['y'] - numpy_y('ContrastFilter', 8, x, f)).max() <= 1e-13
  out['A2_ContrastFilter_features'] = f
  for k in ('params', 'dx', 'dparams', 'dfeatures'):
    out['A2_ContrastFilter_%s' % k] = r[k]

  # ---- B: Tone / Color at cfg.curve_steps 1, 3, 5, 16; x exactly on (L = 16) or at the float64 nearest (3, 5) the knots ---
  for L in (1, 3, 5, 16):
    xb = x.copy()
    knots = np.arange(L + 1) / float(L)
    flat = xb[0].reshape(-1, 3)  # (a view) pixels 20 ..: rows 2, 3 of image 0, behind the constructed pixels of rows 0, 1
    flat[20:20 + L + 1, :] = knots[:, None]
    out['B_L%d_knots' % L] = knots  # x of this case: the forward fixture's x with pixels 20 .. 20 + L of image 0 set to these
    for cls, cc in (('ToneFilter', 1), ('ColorFilter', 3)):
      f = rng.standard_normal((n, cc * L)) * 1.5
      f[0] = 0.0
      r = run_filter(ns0, cls, L, xb, f, dy)
      assert np.abs(r['y'] - numpy_y(cls, L, xb, f)).max() <= 1e-13, (cls, L)
      out['B_L%d_%s_features' % (L, cls)] = f
      for k in ('params', 'y', 'dx', 'dparams', 'dfeatures'):
        out['B_L%d_%s_%s' % (L, cls, k)] = r[k].reshape(n, -1) if k == 'params' else r[k]
      if L in (5, 16):
        r = run_filter(ns0, cls, L, xb, f, dy, dpen=dpen)
        keep_pen('B_L%d_%s' % (L, cls), r)

  # ---- C: masked apply (Filter.get_mask + filters.py:88), cfg.masking on, sharpness 1, minimum strength 0.3 -----------
  for cls in ('ExposureFilter', 'SaturationPlusFilter', 'ContrastFilter', 'ColorFilter'):
    raw = rng.standard_normal((n, 6)) * 1.5
    raw[0] = 0.0
    raw[1] = [20.0, -20.0, 20.0, -20.0, 20.0, -20.0]  # saturated tanh_range
    f = fwd[cls + '_features']
    r = run_filter(ns0, cls, 8, x, f, dy, raw_mask=raw)
    assert np.abs(r['y'] - numpy_y(cls, 8, x, f, raw)).max() <= 1e-13, cls
    out['C_%s_mask_params' % cls] = raw
    for k in ('dx', 'dparams', 'dmask_params'):  # (the forward is checked above and not stored)
      out['C_%s_%s' % (cls, k)] = r[k]

  # ---- D: hsv_grad_mode = 1, SaturationPlus; x without random channels >= 1, plus one v == 0.5 pixel --------------------
  xd = x.copy()
  constructed = np.zeros((n, h, w), dtype=bool)
  constructed[0, 0, :8] = constructed[0, 1, :4] = constructed[1, 0, :4] = constructed[2, 0, :3] = True
  over = (xd >= 1).any(axis=-1) & ~constructed
  xd[over] *= 0.5
  xd[3, 0, 0] = [0.5, 0.25, 0.125]  # v == 0.5: the kink of 0.5 - |0.5 - v|
  xc = np.minimum(xd, 1.0)
  v_, mn_ = xc.max(axis=-1), xc.min(axis=-1)
  ties = (xc[..., 0] == xc[..., 1]) | (xc[..., 1] == xc[..., 2]) | (xc[..., 0] == xc[..., 2])
  smooth = ~(ties | (v_ - mn_ == 0) | (v_ == 0) | (v_ == 0.5) | (xd >= 1).any(axis=-1))
  assert (~smooth).sum() <= 24, (~smooth).sum()
  f = fwd['SaturationPlusFilter_features']
  r = run_filter(ns1, 'SaturationPlusFilter', 8, xd, f, dy)
  assert np.abs(r['y'] - numpy_y('SaturationPlusFilter', 8, xd, f)).max() <= 1e-13
  out['hsv1_x'], out['hsv1_smooth'], out['hsv1_non_smooth_count'] = xd, smooth, np.array(int((~smooth).sum()))
  for k in ('y', 'dx', 'dparams', 'dfeatures'):
    out['hsv1_SaturationPlusFilter_%s' % k] = r[k]

  # ---- E (continued): the cases ---------------------------------------------------------------------------------------------
  def agent_case(tag, logits, states, noise, net, consts, g_s, g_q):
    k = logits.shape[1]
    for is_train in (1, 0):
      acfg = types.SimpleNamespace(exploration=consts[0], test_steps=5, early_stop_penalty=1.0, filter_usage_penalty=1.0,
                                   exploration_penalty=consts[1], clamp=False)
      lt, nt = leaf(logits), leaf(net)
      env = dict(ns0, cfg=acfg, filters=[None] * k, pdf=lt, selection_noise=torch.from_numpy(noise), is_train=is_train,
                 states=torch.from_numpy(states), progress=0.25, net=nt, regular_filter_start=0)
      exec(agent_code, env)
      envn = dict(nsn, cfg=acfg, filters=[None] * k, pdf=logits.copy(), selection_noise=noise, is_train=is_train,
                  states=states, progress=0.25, net=net, regular_filter_start=0)
      exec(agent_code_np, envn)
      for key in ('surrogate', 'penalty', 'selected_filter_id'):
        assert np.abs(npy(env[key]).astype(np.float64) - np.asarray(envn[key], dtype=np.float64)).max() <= 1e-13, key
      name = '%s_%s' % (tag, 'train' if is_train else 'eval')
      if tag == 'agent':
        assert np.abs(npy(env['penalty']) - fwd['%s_penalty' % name]).max() <= 1e-13
        assert np.array_equal(npy(env['selected_filter_id']), fwd['%s_selected_filter_id' % name])
      d_sur, = torch.autograd.grad((env['surrogate'] * torch.from_numpy(g_s)).sum(), [lt], retain_graph=True, allow_unused=True)
      d_sur = torch.zeros_like(lt) if d_sur is None else d_sur
      d_pen, d_net = torch.autograd.grad((env['penalty'] * torch.from_numpy(g_q)).sum(), [lt, nt])
      out[name + '_selected_filter_id'] = npy(env['selected_filter_id']).astype(np.int32)
      out[name + '_d_logits_surrogate'], out[name + '_d_logits_penalty'] = npy(d_sur), npy(d_pen)
      out[name + '_d_logits'] = npy(d_sur + d_pen)
      out[name + '_d_net'] = npy(d_net)

  f32r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # the cotangents are exactly representable in fp32
  m = fwd['agent_logits'].shape[0]
  g_s, g_q = f32r(rng.standard_normal((m, 1))), f32r(rng.standard_normal((m, 1)))
  out['agent_g_s'], out['agent_g_q'] = g_s, g_q
  base = (fwd['agent_logits'], fwd['agent_states'], fwd['agent_noise'], fwd['agent_net'])
  agent_case('agent', *base, (0.05, 0.05), g_s, g_q)  # config_example.py:48-69
  agent_case('agentx', *base, (0.0625, 0.0625), g_s, g_q)  # constants that float32 holds exactly
  for k in (5, 12):
    mk = 12
    logits = rng.standard_normal((mk, k)) * 2
    logits[1] = 0.75  # an all-equal row
    logits[2] = np.linspace(0, 120, k)  # softmax underflows: the 1e-37 / 1e-30 / 1e-10 guards enter the gradient
    states = np.zeros((mk, 3 + k))
    states[:, 2] = rng.integers(0, 6, mk)
    states[:, 3:] = (rng.random((mk, k)) < 0.3).astype(np.float64)
    noise = rng.random((mk, 1))
    noise[0, 0] = 0.0
    net = rng.random((mk, 6, 5, 3)) * 1.3
    gs_k, gq_k = f32r(rng.standard_normal((mk, 1))), f32r(rng.standard_normal((mk, 1)))
    tag = 'agentK%d' % k
    for key, val in (('logits', logits), ('states', states), ('noise', noise), ('net', net), ('g_s', gs_k), ('g_q', gq_k)):
      out['%s_%s' % (tag, key)] = val
    agent_case(tag, logits, states, noise, net, (0.05, 0.05), gs_k, gq_k)

  # ---- F: util.lrelu' (0.6 x + 0.4 |x| with abs'(0) = 0: 0.6 at 0, -0.0 and nowhere else) -------------------------------
  xs = leaf(fwd['util_lrelu_x'])
  ys = ns0['lrelu'](xs)
  assert np.abs(npy(ys) - fwd['util_lrelu_y']).max() <= 1e-15
  out['util_lrelu_dx'] = npy(torch.autograd.grad(ys.sum(), [xs])[0])

  out['standin_ops'] = np.array(sorted(ns0['tf'].used))
  out['standin_ops_hsv1'] = np.array(sorted(ns1['tf'].used))
  out['rewrites'] = np.array(REWRITES)
  out['pen_is_plain'] = np.array(pen_is_plain)
  out['provenance'] = np.array(['%s sha256=%s' % p for p in prov])
  path = os.path.join(HERE, 'reference_grad_facade.npz')
  save_deterministic(path, out)
  print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
  print('stand-in ops:', ', '.join(sorted(ns0['tf'].used)))
  print('non-smooth pixels of case D: %d' % int((~smooth).sum()))


def save_deterministic(path, arrays):
  """np.savez_compressed with fixed zip timestamps: the same arrays give the same bytes."""
  import io
  import zipfile
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
    for key in arrays:
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
      info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      z.writestr(info, buf.getvalue())


if __name__ == '__main__':
  if not os.path.isdir(REF):
    sys.exit('needs /root/reference (the build container)')
  main()
