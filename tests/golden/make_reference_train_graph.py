"""TRAINING-GRAPH COMPOSITION PIN -- TF primitives and their gradients ASSUMED and listed.  It pins no primitive.

The sibling of make_reference_grad_facade.py for the graph AROUND the filters.  Cut out of the reference's files by ``ast``
at generation time and EXECUTED under a torch stand-in for ``tf`` / ``ly`` (float64, autograd on, ``create_graph`` for the
gradient penalty's inner ``tf.gradients``) -- no line of the reference is copied here:

  K  networks    the whole functions critics.cnn and critics.critic (without states, and with states inside
                 variable_scope('rl_value')), agent.feature_extractor, util.enrich_image_input and the classes
                 filters.Filter + the eight of config_example.py:22-25 (extract_parameters among their methods)
  L  loss graph  the statements of net.GAN.__init__ from the first cfg.critic(...) call to the end of the
                 gradient-penalty block (found by their assignment targets), on leaf tensors fake_output, new_states,
                 surrogate_loss_addition, penalty; ``self`` a plain namespace, cfg.critic = cfg.value = K's function
  G  one step    agent.agent_generator (is_train = 1, masking off) wired through the statements of net.py's
                 ``with tf.variable_scope('generator')`` block into L

Two configurations (tests/_train_graph_ref.py): S stores everything in float64; P (the shipped sizes) stores scalars,
logits, bias and image gradients in full and every weight gradient as norm, sum and a strided sample (float32).

The stand-in's conventions (written into the fixture as ``standin_ops``): SAME padding with the extra pixel after,
cross-correlation, HWIO kernels and (in, out) matrices, NHWC flatten, reduce_max / reduce_min split the gradient evenly
between tied extrema, clip_by_value passes on lo <= x <= hi, minimum(x, y) sends ties to x, maximum(x, c) passes on
x >= c, abs'(0) = 0, tf.nn.moments takes the variance around stop_gradient(mean) (as TF does), dropout is
x / keep_prob * mask with supplied masks, TF-1 default-name uniquification (Conv, Conv_1, ...; fully_connected,
fully_connected_1) that restarts when a named scope is entered again.

``f32_floor``: the same graphs once more with the stand-in in float32 on the CPU -- per tensor, the worst difference from
the float64 result over that tensor's largest magnitude: the noise floor of float32 arithmetic on the reference's own
graph, which the GPU tests' bounds are built from.

  python tests/golden/make_reference_train_graph.py        # rewrites tests/golden/reference_train_graph_{S,S_K,S_L,S_G,P_L,P_G}.npz
"""
import ast
import contextlib
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE_ = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE_)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE_)))
from make_reference_facade import HERE, REF, cut_span, no_prints, sha256  # noqa: E402
from make_reference_grad_facade import NoAugAssign, TorchTf, save_deterministic  # noqa: E402
from tests import _train_graph_ref as R  # noqa: E402

FILTER_CLASSES = ['ExposureFilter', 'GammaFilter', 'ImprovedWhiteBalanceFilter', 'SaturationPlusFilter', 'ToneFilter',
                  'ContrastFilter', 'WNBFilter', 'ColorFilter']  # config_example.py:22-25

REWRITES = [
    'AugAssign -> Assign in every cut body (value-identical; autograd has saved the tensors written in place)',
    'np.array -> tensor of the stand-in\'s dtype; builtin abs -> the stand-in\'s abs (abs\'(0) = 0)',
    'torch.Tensor gets get_shape() -> .shape for the duration of the script (critics.py:9, agent.py:16, filters.py:13)',
    'print -> no-op',
]


# ---- TF conventions as explicit autograd functions (differentiable twice: the backward formulas are linear in g) ----------
class _ReduceExtreme(torch.autograd.Function):
  """tf.reduce_max / reduce_min over one axis: the gradient is split evenly between tied extrema."""

  @staticmethod
  def forward(ctx, x, dim, is_max):
    xd = x.detach()
    m = xd.amax(dim=dim, keepdim=True) if is_max else xd.amin(dim=dim, keepdim=True)
    sel = (xd == m).to(x.dtype)
    ctx.save_for_backward(sel / sel.sum(dim=dim, keepdim=True))
    ctx.dim = dim
    return m.squeeze(dim)

  @staticmethod
  def backward(ctx, g):
    return g.unsqueeze(ctx.dim) * ctx.saved_tensors[0], None, None


class _MinXY(torch.autograd.Function):
  """tf.minimum(x, y) of two tensors: the gradient goes to x where x <= y, else to y."""

  @staticmethod
  def forward(ctx, x, y):
    ctx.save_for_backward((x <= y).to(x.dtype))
    return torch.minimum(x.detach(), y.detach())

  @staticmethod
  def backward(ctx, g):
    to_x, = ctx.saved_tensors
    return g * to_x, g * (1.0 - to_x)


class VarStore:
  """TF-1 variable scopes: names, default-name uniquification per scope (restarting when a named scope is entered
  again), reuse.  Variables are leaf tensors made from supplied arrays, in the order the text creates them."""

  def __init__(self, weights, dtype):
    self.weights, self.dtype = weights, dtype
    self.vars, self.created = {}, []
    self.path, self.reuse, self.counts = [], False, {}

  def prefix(self):
    return ''.join(p + '/' for p in self.path)

  @contextlib.contextmanager
  def scope(self, name):
    outer_reuse = self.reuse
    self.path.append(name)
    store = self

    class Handle:

      def reuse_variables(self):
        store.reuse = True

    try:
      yield Handle()
    finally:
      full = self.prefix()
      for key in [k for k in self.counts if k.startswith(full)]:
        del self.counts[key]
      self.path.pop()
      self.reuse = outer_reuse

  def default_scope(self, default):
    c = self.counts.setdefault(self.prefix(), {})
    k = c.get(default, 0)
    c[default] = k + 1
    return default if k == 0 else '%s_%d' % (default, k)

  def get(self, name, shape):
    full = self.prefix() + name
    if self.reuse:
      assert full in self.vars, 'reuse of a variable that does not exist: ' + full
      assert tuple(self.vars[full].shape) == tuple(shape), full
      return self.vars[full]
    assert full not in self.vars, 'variable exists and reuse is off: ' + full
    a = np.asarray(self.weights[full], dtype=np.float64)
    assert a.shape == tuple(shape), (full, a.shape, tuple(shape))
    v = torch.tensor(a, dtype=self.dtype, requires_grad=True)
    self.vars[full] = v
    self.created.append((full, tuple(shape)))
    return v


class TrainTf(TorchTf):
  """make_reference_grad_facade.TorchTf in a chosen dtype, plus the primitives of critics.py, agent.py:11-99 and
  net.py:68-199."""

  int32 = torch.int32

  def __init__(self, store, dtype, alpha, dropout_masks):
    super().__init__(0)
    self.store, self.dt, self.float32 = store, dtype, dtype
    self.alpha, self.masks = alpha, list(dropout_masks)
    self.min_preact = float('inf')
    facade, base_image, base_nn = self, self.image, self.nn

    class image:
      rgb_to_hsv = staticmethod(lambda x: base_image.rgb_to_hsv(x).to(dtype))
      hsv_to_rgb = staticmethod(lambda x: base_image.hsv_to_rgb(x).to(dtype))

    class nn:
      softmax = base_nn.softmax

      @staticmethod
      def moments(x, axes, keep_dims=False):
        facade._u('nn.moments [population variance around stop_gradient(mean)]')
        mean = x.mean(dim=tuple(axes), keepdim=True)
        var = ((x - mean.detach())**2).mean(dim=tuple(axes), keepdim=True)
        if not keep_dims:
          mean, var = mean.reshape(mean.shape[0]), var.reshape(var.shape[0])
        return mean, var

      @staticmethod
      def dropout(x, keep_prob):
        facade._u('nn.dropout [x / keep_prob * mask, supplied masks in call order]')
        return x / keep_prob * facade.masks.pop(0)

    class Uniform:

      def __init__(self, low, high):
        assert (low, high) == (0., 1.)

      def sample(self, shape):
        facade._u('contrib.distributions.Uniform.sample [the supplied alpha]')
        assert tuple(shape) == tuple(facade.alpha.shape), (shape, facade.alpha.shape)
        return facade.alpha

    class Ema:

      def __init__(self, decay, zero_debias):
        pass

      def apply(self, values):
        return None

      def average(self, value):
        return value.detach() * 0

    self.image, self.nn = image, nn
    self.contrib = types.SimpleNamespace(distributions=types.SimpleNamespace(Uniform=Uniform),
                                         layers=types.SimpleNamespace(xavier_initializer=lambda: None))
    self.train = types.SimpleNamespace(ExponentialMovingAverage=Ema)
    self.summary = types.SimpleNamespace(scalar=lambda *a, **k: None)

  def variable_scope(self, name):
    return self.store.scope(name)

  def constant(self, x, dtype=None):
    self._u('constant')
    return torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=self.dt)

  def ones(self, shape, dtype=None):
    self._u('ones')
    return torch.ones(tuple(shape), dtype=self.dt)

  def clip_by_value(self, x, clip_value_min, clip_value_max):  # (critics.py:55-58 spells the bounds as keywords)
    return super().clip_by_value(x, clip_value_min, clip_value_max)

  def minimum(self, x, y):
    if torch.is_tensor(y):
      self._u('minimum [two tensors: ties to x]')
      return _MinXY.apply(x, y)
    return super().minimum(x, y)

  def reduce_max(self, x, reduction_indices):
    self._u('reduce_max [even split between tied extrema]')
    (dim,) = reduction_indices
    return _ReduceExtreme.apply(x, dim, True)

  def reduce_min(self, x, reduction_indices):
    self._u('reduce_min [even split between tied extrema]')
    (dim,) = reduction_indices
    return _ReduceExtreme.apply(x, dim, False)

  def reshape(self, x, shape):
    self._u('reshape [row-major: NHWC flattens as (H, W, C)]')
    return torch.reshape(x, tuple(int(s) for s in shape))

  def tile(self, x, multiples):
    self._u('tile')
    return x.repeat(*multiples)

  def stack(self, values, axis):
    self._u('stack')
    return torch.stack(list(values), dim=axis)

  def sqrt(self, x): self._u('sqrt'); return torch.sqrt(x)
  def stop_gradient(self, x): self._u('stop_gradient'); return x.detach()

  def cast(self, x, dtype):
    self._u('cast')
    return x.to(dtype)

  def gradients(self, ys, xs):
    self._u('gradients [autograd.grad from ones, create_graph]')
    return list(torch.autograd.grad(ys, xs, torch.ones_like(ys), create_graph=True))


class Ly:
  """tensorflow.contrib.layers: conv2d (padding SAME, kernels HWIO, cross-correlation) and fully_connected ((in, out))."""

  def __init__(self, tf):
    self.tf = tf

  def _act(self, pre, activation_fn):
    if activation_fn is None:
      return pre
    self.tf.min_preact = min(self.tf.min_preact, float(pre.detach().abs().min()))
    return activation_fn(pre)

  def conv2d(self, net, num_outputs, kernel_size, stride, activation_fn=None, normalizer_fn=None, normalizer_params=None):
    tf, store = self.tf, self.tf.store
    tf._u('ly.conv2d [SAME: out = ceil(in / s), the extra pixel after; cross-correlation; HWIO; default scope Conv]')
    assert normalizer_fn is None
    num_outputs = int(num_outputs)
    assert num_outputs == num_outputs // 1
    with store.scope(store.default_scope('Conv')):
      w = store.get('weights', (kernel_size, kernel_size, int(net.shape[3]), num_outputs))
      b = store.get('biases', (num_outputs,))
    pads = []
    for size in (int(net.shape[2]), int(net.shape[1])):  # F.pad: last dimension first
      out = -(-size // stride)
      total = max((out - 1) * stride + kernel_size - size, 0)
      pads += [total // 2, total - total // 2]
    x = F.pad(net.permute(0, 3, 1, 2), pads)
    y = F.conv2d(x, w.permute(3, 2, 0, 1), b, stride=stride).permute(0, 2, 3, 1)
    return self._act(y, activation_fn)

  def fully_connected(self, net, num_outputs, activation_fn=None, scope=None, weights_initializer=None):
    tf, store = self.tf, self.tf.store
    tf._u('ly.fully_connected [x @ w + b, w (in, out); default scope fully_connected]')
    name = scope if scope is not None else store.default_scope('fully_connected')
    with store.scope(name):
      w = store.get('weights', (int(net.shape[1]), int(num_outputs)))
      b = store.get('biases', (int(num_outputs),))
    return self._act(net @ w + b, activation_fn)


class NpShim:
  """``np`` as the cut bodies see it: ``array`` gives a tensor of the stand-in's dtype, the rest is NumPy."""

  def __init__(self, dtype):
    self._dt = dtype

  def array(self, obj, dtype=None):
    return torch.as_tensor(np.array(obj, dtype=np.float64), dtype=self._dt)

  def __getattr__(self, name):
    return getattr(np, name)


def compile_tree(body, name):
  tree = NoAugAssign().visit(ast.Module(body=list(body), type_ignores=[]))
  ast.fix_missing_locations(tree)
  return compile(tree, name, 'exec')


def targets_of(stmt):
  return ast.unparse(stmt.targets[0]) if isinstance(stmt, ast.Assign) else ''


def cut_reference():
  """-> (code objects, provenance)."""
  paths = {n: os.path.join(REF, n) for n in ('util.py', 'filters.py', 'pdf_sample_layer.py', 'agent.py', 'critics.py', 'net.py')}
  prov = ['%s sha256=%s' % (n, sha256(p)) for n, p in paths.items()]
  parse = lambda n: ast.parse(open(paths[n]).read(), filename=paths[n])
  defs = lambda tree, kind, names: [nd for nd in tree.body if isinstance(nd, kind) and nd.name in names]
  code = {}
  util = []
  for name in ('lrelu', 'rgb2lum', 'tanh01', 'tanh_range', 'lerp', 'enrich_image_input'):
    util += cut_span(paths['util.py'], name).body
  code['util'] = compile_tree(util, '<reference util.py functions>')
  classes = defs(parse('filters.py'), ast.ClassDef, ['Filter'] + FILTER_CLASSES)
  assert len(classes) == 9
  code['filters'] = compile_tree(classes, '<reference filters.py classes>')
  code['pdf'] = compile_tree(defs(parse('pdf_sample_layer.py'), ast.FunctionDef, ['pdf_sample']), '<reference pdf_sample>')
  agent = defs(parse('agent.py'), ast.FunctionDef, ['feature_extractor', 'agent_generator'])
  assert len(agent) == 2
  code['agent'] = compile_tree(agent, '<reference agent.py functions>')
  critics = defs(parse('critics.py'), ast.FunctionDef, ['cnn', 'critic'])
  assert len(critics) == 2
  code['critics'] = compile_tree(critics, '<reference critics.py functions>')
  gan = next(nd for nd in parse('net.py').body if isinstance(nd, ast.ClassDef) and nd.name == 'GAN')
  init = next(fn for fn in gan.body if isinstance(fn, ast.FunctionDef) and fn.name == '__init__')
  body = init.body
  # G's wiring: the `with tf.variable_scope('generator')` block and the assignment in front of it
  i_gen = next(i for i, s in enumerate(body) if isinstance(s, ast.With) and 'generator' in ast.unparse(s.items[0]))
  assert targets_of(body[i_gen - 1]) == 'self.surrogate_loss_addition'
  code['net_generator'] = compile_tree(body[i_gen - 1:i_gen + 1], '<reference net.py generator block>')
  # L: from the assignment whose targets start with self.real_logit to the `if` behind self.critic_gradient_norm
  i_first = next(i for i, s in enumerate(body) if targets_of(s).startswith('(self.real_logit,'))
  assert 'cfg.critic(' in ast.unparse(body[i_first]) and i_first > i_gen
  i_norm = next(i for i, s in enumerate(body) if targets_of(s) == 'self.critic_gradient_norm')
  i_last = next(i for i in range(i_norm, len(body)) if isinstance(body[i], ast.If))
  assert "cfg.gan == 'w'" in ast.unparse(body[i_last].test)
  assert not any('cfg.critic(' in ast.unparse(s) for s in body[:i_first])
  code['net_losses'] = compile_tree(no_prints(body[i_first:i_last + 1]), '<reference net.py loss graph>')
  return code, prov


class Graph:
  """One namespace with the cut functions executed in it, over one variable store."""

  def __init__(self, code, tag, weights, inp, dtype):
    self.tag, self.inp, self.dtype = tag, inp, dtype
    self.store = VarStore(weights, dtype)
    self.t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    self.tf = TrainTf(self.store, dtype, self.t(inp['alpha']), [self.t(m) for m in inp['dropout_masks']])
    ns = {'tf': self.tf, 'ly': Ly(self.tf), 'math': math, 'np': NpShim(dtype), 'abs': self.tf.abs, 'cv2': None,
          'print': lambda *a, **k: None, 'STATE_REWARD_DIM': 0, 'STATE_STOPPED_DIM': 1, 'STATE_STEP_DIM': 2,
          'STATE_DROPOUT_BEGIN': 3}
    for key in ('util', 'filters', 'pdf', 'agent', 'critics'):
      exec(code[key], ns)
    self.ns, self.code = ns, code
    s = R.SIZES[tag]
    self.cfg = types.SimpleNamespace(
        # config_example.py, values only
        filters=[ns[c] for c in FILTER_CLASSES], curve_steps=8, gamma_range=3, exposure_range=3.5, wb_range=1.1,
        color_curve_range=(0.90, 1.10), lab_curve_range=(0.90, 1.10), tone_curve_range=(0.5, 2), masking=False,
        minimum_strength=0.3, maximum_sharpness=1, clamp=False, critic_logit_multiplier=0.05, discount_factor=1.0,
        filter_usage_penalty=1.0, use_TD=True, maximum_trajectory_length=7, all_reward=1.0, img_include_states=True,
        exploration=0.05, exploration_penalty=0.05, early_stop_penalty=1.0, dropout_keep_prob=0.5,
        shared_feature_extractor=True, use_penalty=True, gan='w', generator=ns['agent_generator'], critic=ns['critic'],
        value=ns['critic'], gradient_penalty_lambda=10, test_steps=5, supervised=False, batch_size=R.N, parameter_lr_mul=1,
        **s)
    # the values typed above against the ones recorded from the reference's config_example.py (reference_config.json)
    import json
    recorded = json.load(open(os.path.join(HERE, 'reference_config.json')))['config_example.py']
    assert FILTER_CLASSES == recorded['other']['filters']
    checked = 0
    for key, want in recorded['plain'].items():
      if hasattr(self.cfg, key) and key not in tuple(s) + ('batch_size',):
        got = getattr(self.cfg, key)
        assert (list(got) if isinstance(got, tuple) else got) == want, (key, got, want)
        checked += 1
    assert checked >= 29, checked  # every field typed above that the reference config holds as plain data

  def leaf(self, a):
    return self.t(a).requires_grad_(True)

  def theta(self, scope):
    return [(n, self.store.vars[n]) for n, _ in self.store.created if n.startswith(scope)]

  def losses(self, self_):
    """L: the statements of net.py on a namespace ``self_`` that holds the inputs."""
    self_.cfg, self_.is_training = self.cfg, True
    env = dict(self.ns, self=self_, cfg=self.cfg)
    exec(self.code['net_losses'], env)
    self.env = env
    return self_


def npy(t):
  return t.detach().to(torch.float64).numpy().copy()


def grads_of(loss, named):
  g = torch.autograd.grad(loss, [v for _, v in named], retain_graph=True, allow_unused=True)
  return {n: (np.zeros(tuple(v.shape)) if gi is None else npy(gi)) for (n, v), gi in zip(named, g)}


SCALARS = ('g_loss', 'v_loss', 'c_loss', 'emd', 'c_average', 'critic_gradient_norm')
PER_IMAGE = ('reward', 'q_value', 'advantage', 'fake_logit', 'real_logit', 'fake_input_logit', 'old_value', 'new_value')


def record_losses(out, pre, g, s, leaves):
  for k in SCALARS + PER_IMAGE:
    out[pre + k] = npy(getattr(s, k))
  out[pre + 'gradient_penalty'] = out[pre + 'c_loss'] + out[pre + 'emd']  # c_loss = -emd + penalty (net.py:164, 194)
  out[pre + 'gradient_norms'] = npy(g.env['gradient_norm'])  # (locals of the text, per interpolate)
  if pre == 'L_':
    out[pre + 'gradients'] = npy(g.env['gradients'])
  for n, a in grads_of(s.c_loss, g.theta('critic/')).items():
    out[pre + 'dc_loss/' + n] = a
  for n, a in grads_of(s.v_loss, g.theta('rl_value/')).items():
    out[pre + 'dv_loss/' + n] = a
  for n, a in grads_of(s.g_loss, leaves).items():
    out[pre + 'dg_loss/' + n] = a


def run_K(code, tag, weights, inp, dtype):
  g = Graph(code, tag, weights, inp, dtype)
  ns, cfg, out = g.ns, g.cfg, {}
  c = g.t(inp['logit_cotangent'])
  img, st = g.leaf(inp['fake_input']), g.leaf(inp['states'])
  logit, _, _ = ns['critic'](images=img, cfg=cfg, is_train=True)
  out['K_critic_logit'] = npy(logit)
  for n, a in grads_of((logit * c).sum(), [('images', img)] + g.theta('critic/')).items():
    out['K_critic_d/' + n] = a
  with g.tf.variable_scope('rl_value'):
    value, _, _ = ns['critic'](images=img, states=st, cfg=cfg, reuse=False, is_train=True)
  out['K_value_logit'] = npy(value)
  for n, a in grads_of((value * c).sum(), [('images', img), ('states', st)] + g.theta('rl_value/')).items():
    out['K_value_d/' + n] = a
  # feature_extractor on enrich_image_input, then Filter.extract_parameters of the last filter (ColorFilter: 24 + 6)
  with g.tf.variable_scope('generator'):
    feat = ns['feature_extractor'](net=ns['enrich_image_input'](cfg, img, st), output_dim=cfg.feature_extractor_dims, cfg=cfg)
    with g.tf.variable_scope('filter_7'):
      f, m = ns['ColorFilter'](img, cfg).extract_parameters(feat)
  out['K_features'], out['K_filter7_features'], out['K_filter7_mask_parameters'] = npy(feat), npy(f), npy(m)
  cot = g.t(np.cos(np.arange(f.shape[0] * (f.shape[1] + m.shape[1]))).reshape(f.shape[0], -1))
  for n, a in grads_of((torch.cat([f, m], dim=1) * cot).sum(), [('images', img), ('states', st)] + g.theta('generator/')).items():
    out['K_extract_d/' + n] = a
  out['K_extract_cotangent'] = npy(cot)
  return out, g


def run_L(code, tag, weights, inp, dtype):
  g = Graph(code, tag, weights, inp, dtype)
  s = types.SimpleNamespace(real_data=g.t(inp['real_data']), fake_input=g.t(inp['fake_input']), states=g.t(inp['states']),
                            fake_output=g.leaf(inp['fake_output']), new_states=g.leaf(inp['new_states']),
                            surrogate_loss_addition=g.leaf(inp['surrogate']), penalty=g.leaf(inp['penalty']))
  g.losses(s)
  out = {}
  leaves = [('fake_output', s.fake_output), ('new_states', s.new_states), ('surrogate_loss_addition', s.surrogate_loss_addition),
            ('penalty', s.penalty)]
  record_losses(out, 'L_', g, s, leaves)
  return out, g, s


def run_G(code, tag, weights, inp, dtype):
  g = Graph(code, tag, weights, inp, dtype)
  memory = types.SimpleNamespace()
  s = types.SimpleNamespace(real_data=g.t(inp['real_data']), fake_input=g.t(inp['fake_input']), states=g.t(inp['states']),
                            z=g.t(inp['z']), is_train=1, progress=float(inp['progress']), fake_input_feature=None, memory=memory)
  # what the text itself hands to and gets from pdf_sample (agent.py:113): the action pdf, the noise, the sampled ids
  sample, g.sampled = g.ns['pdf_sample'], []

  def spy(pdf, noise):
    ids = sample(pdf, noise)
    g.sampled.append((npy(pdf), npy(noise), npy(ids).astype(np.int32)))
    return ids

  g.ns['pdf_sample'] = spy
  exec(g.code['net_generator'], dict(g.ns, self=s, cfg=g.cfg))
  g.ns['pdf_sample'] = sample
  g.losses(s)
  out = {}
  record_losses(out, 'G_', g, s, g.theta('generator/'))
  out['G_fake_output'], out['G_new_states'] = npy(s.fake_output), npy(s.new_states)
  out['G_surrogate'], out['G_penalty'] = npy(s.surrogate_loss_addition), npy(s.penalty)
  return out, g, s


def g_extras(out, g, s, inp):
  """The selected ids, the action pdf and the distance of the selection noise from the cumulative pdf's edges, all from
  the one call of pdf_sample that the executed agent_generator made (run_G's spy; is_train = 1, so the sampled ids are the
  selected ones, agent.py:115-116).  Cross-checked against the text's own new_states: the usage bits that changed are
  the selected filters', and every selected filter's bit is set."""
  (pdf, noise, ids), = g.sampled
  assert np.array_equal(noise, inp['z'][:, 0:1])
  usage, new_usage = inp['states'][:, 3:], out['G_new_states'][:, 3:]
  one_hot = ids[:, None] == np.arange(R.NUM_FILTERS)[None, :]
  assert np.array_equal(new_usage, np.maximum(usage, one_hot)), 'the ids do not explain the text\'s new_states'
  assert (new_usage - usage != 0).any(axis=1).sum() >= 2  # (a filter used before leaves no trace: not every row can show it)
  cdf = np.concatenate([np.zeros((R.N, 1)), np.cumsum(pdf / (pdf.sum(axis=1, keepdims=True) + 1e-36), axis=1)], axis=1)
  margin = np.abs(cdf - noise).min()
  out['G_selected_filter_id'], out['G_pdf'], out['G_noise_margin'] = ids, pdf, np.array(margin)
  return ids, margin


def floors(ref, low):
  names, vals = [], []
  for k in sorted(ref):
    a, b = ref[k], low[k]
    if a.dtype.kind != 'f' or a.size == 0:
      continue
    scale = np.abs(a).max()
    names.append(k)
    vals.append(0.0 if scale == 0 else np.abs(a - b).max() / scale)
  return np.array(names), np.array(vals)


def configuration(code, prov, tag):
  inp = R.inputs(tag)
  # ---- the critic's last layer: scaled so that the interpolates' gradient norms lie on both sides of 1 --------------------
  w1 = R.weights(tag)
  _, g1, s1 = run_L(code, tag, w1, inp, torch.float64)
  raw = npy(g1.env['gradient_norm'])  # (linear in the scale up to the 1e-6 under the root)
  order = np.sort(raw)
  # between the second and the third norm (geometric mean), as a power of two times an 8-bit mantissa: exact in fp32
  scale = float(np.float32(1.0 / math.sqrt(order[1] * order[2])))
  scale = float(np.round(scale * 2.0**(8 - math.floor(math.log2(scale)))) / 2.0**(8 - math.floor(math.log2(scale))))
  weights = R.weights(tag, critic_fc2_scale=scale)
  assert list(weights) == [n for n, _ in R.variable_shapes(tag)]

  out = dict(critic_fc2_scale=np.array(scale))
  res = {}
  for name, fn in (('K', run_K), ('L', run_L), ('G', run_G)):
    res[name] = fn(code, tag, weights, inp, torch.float64)
    out.update(res[name][0])
  ids, margin = g_extras(out, res['G'][1], res['G'][2], inp)
  low = {}
  for name, fn in (('K', run_K), ('L', run_L), ('G', run_G)):
    r32 = fn(code, tag, weights, inp, torch.float32)
    low.update(r32[0])
    if name == 'G':
      assert np.array_equal(npy(r32[2].new_states), out['G_new_states']), 'float32 takes another discrete outcome'
  out['f32_floor_names'], out['f32_floor'] = floors({k: v for k, v in out.items() if k in low}, low)

  # ---- the asserts that let the float64 reference alone fix every discrete outcome ---------------------------------------
  for key in ('real_data', 'fake_input', 'fake_output'):
    x = inp[key]
    assert np.array_equal(x * 1024, np.round(x * 1024)) and x.min() >= -0.1 and x.max() <= 1.25, key
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x), key
    px = x.reshape(R.N, -1, 3)
    assert (px[:, 0, 0] == px[:, 0, 1]).all() and (px[:, 0, 1] == px[:, 0, 2]).all() and (px[:, 4, 0] == px[:, 4, 1]).all()
    assert (px[:, 8, 2] == 1).all() and (px[:, 12, 0] == 0).all() and (px[:, 16].max(axis=1) + px[:, 16].min(axis=1) == 1).all()
  ns_ = inp['new_states']
  assert set(ns_[:, 1]) == {0.0, 1.0} and (ns_[:, 2] > 7).any() and (ns_[:, 2] <= 7).any()
  gs = out['G_new_states']
  assert set(gs[:, 1]) == {0.0, 1.0} and (gs[:, 2] > 7).any() and (gs[:, 2] <= 7).any()
  norms = out['L_gradient_norms']
  assert (norms > 1 + 1e-3).any() and (norms < 1 - 1e-3).any() and (np.abs(norms - 1) > 1e-3).all(), norms
  assert (np.abs(out['G_gradient_norms'] - 1) > 1e-3).all() and out['G_gradient_penalty'] > 0, out['G_gradient_norms']
  assert margin >= 1e-3, margin
  for name in ('K', 'L', 'G'):
    assert res[name][1].tf.min_preact >= 1e-9, (name, res[name][1].tf.min_preact)
  out['min_preactivation'] = np.array(min(res[n][1].tf.min_preact for n in res))
  created = res['G'][1].store.created
  assert sorted(created) == sorted(R.variable_shapes(tag)), 'tests/_train_graph_ref.py::variable_shapes is not what the text creates'
  assert sorted(res['L'][1].store.created) == sorted(c for c in created if not c[0].startswith('generator/'))
  out['variable_names'] = np.array([n for n, _ in created])
  out['variable_shapes'] = np.array([' '.join(str(d) for d in sh) for _, sh in created])
  ops = set()
  for name in res:
    ops |= res[name][1].tf.used
  out['standin_ops'] = np.array(sorted(ops))
  out['rewrites'] = np.array(REWRITES)
  out['provenance'] = np.array(prov)
  out['weights_sha256'] = np.array(R.weights_sha256(weights))
  out['inputs_sha256'] = np.array(R.inputs_sha256(inp))
  print('%s: fc2 scale %r, interpolates\' norms %s, selected ids %s, noise margin %.4f, min |pre-activation| %.3g' %
        (tag, scale, np.round(norms, 4), ids, margin, float(out['min_preactivation'])))
  return out, weights, inp


def compact(out):
  """P: weight gradients as (norm, sum, every k-th entry in float32); everything else as it is."""
  small = {}
  for k, a in out.items():
    if k.startswith('K_') or k.startswith('G_dc_loss/'):
      continue  # (the networks alone are pinned at S; the critic's update is compared on L)
    if '/' in k and k.endswith('/weights'):
      flat = a.reshape(-1)
      small[k + ':norm'] = np.array(np.sqrt((flat**2).sum()))
      small[k + ':sum'] = np.array(flat.sum())
      small[k + ':max'] = np.array(np.abs(flat).max())
      small[k + ':sample'] = flat[::R.sample_stride(flat.size)].astype(np.float32)
    elif a.dtype.kind == 'f' and a.size > 4096:
      small[k] = a.astype(np.float32)  # images and image gradients
    else:
      small[k] = a
  return small


def build(tag, code=None, prov=None):
  """One thread: the order of torch's sums, and with it the last bits, would follow the thread count."""
  if code is None:
    code, prov = cut_reference()
  threads = torch.get_num_threads()
  torch.set_num_threads(1)
  try:
    out, weights, inp = configuration(code, prov, tag)
  finally:
    torch.set_num_threads(threads)
  if tag == 'S':
    for k, a in weights.items():
      out['weight/' + k] = a
    for k, a in inp.items():
      out['input/' + k] = a
    return out
  return compact(out)


def main():
  torch.Tensor.get_shape = lambda self: self.shape
  code, prov = cut_reference()
  for tag in ('S', 'P'):
    out = build(tag, code, prov)
    # several files each (inputs / weights / loss graph, the networks, the whole step): every one below the largest fixture
    # committed before
    part = lambda keep: {k: v for k, v in out.items() if keep(k)}
    if tag == 'S':
      parts = {'S': part(lambda k: k[:2] not in ('K_', 'L_', 'G_')), 'S_K': part(lambda k: k[:2] == 'K_'),
               'S_L': part(lambda k: k[:2] == 'L_'), 'S_G': part(lambda k: k[:2] == 'G_')}
    else:
      parts = {'P_L': part(lambda k: k[:2] != 'G_'), 'P_G': part(lambda k: k[:2] != 'L_')}
    for name, arrays in parts.items():
      path = os.path.join(HERE, 'reference_train_graph_%s.npz' % name)
      save_deterministic(path, arrays)
      print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
  if not os.path.isdir(REF):
    sys.exit('needs the reference checkout')
  main()
