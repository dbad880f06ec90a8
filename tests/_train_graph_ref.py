"""Shared by tests/golden/make_reference_train_graph.py (which records) and tests/test_reference_train_graph.py (which
compares): the two configurations, the variables a configuration's graph holds, and the deterministic draws of weights and
inputs.  Nothing here computes a network or a loss.

S: config_example.py's values with source_img_size 32, base_channels 8, fc1_size 16, feature_extractor_dims 256 -- three
convolutions per net, both arms of feature_extractor's channel rule (agent.py:25-28), 512 critic features.  P: the shipped
sizes (64 x 64, 32 channels, 128, 4096).  N = 4 images in both."""
import hashlib

import numpy as np

N = 4
NUM_FILTERS = 8
FILTER_PARAMS = (1, 1, 3, 1, 8, 1, 1, 24)  # config_example.py:22-27 in cfg.filters order, curve_steps = 8
SIZES = {
    'S': dict(source_img_size=32, base_channels=8, fc1_size=16, feature_extractor_dims=256),
    'P': dict(source_img_size=64, base_channels=32, fc1_size=128, feature_extractor_dims=4096),
}
SEEDS = {'S': 20261021, 'P': 20261022}
PROGRESS = 0.25  # exact in float32
# one noise per image, in the middle of an eighth of [0, 1]: near-uniform action pdfs then pick four different filters
SELECTION_NOISE = (0.0625, 0.3125, 0.5625, 0.9375)
STEPS = (6.0, 4.0, 2.0, 7.0)       # G: the step counters of `states` (4 + 1 == test_steps: submits; 6 + 1 == the trajectory length: kept; 7 + 1: cleared)
L_STEPS = (7.0, 8.0, 5.0, 9.0)     # L: the step counters of the leaf `new_states`: on maximum_trajectory_length (kept: `>`) and past it
L_STOPPED = (0.0, 0.0, 1.0, 1.0)


def oracle_cfg(tag):
  """The dict oracle/nets_np.py takes."""
  from oracle import nets_np
  return dict(nets_np.DEFAULT_CFG, **SIZES[tag])


def product_cfg(tag):
  """The cfg exposure_amd.gan.GAN takes."""
  from exposure_amd.config import make_cfg
  cfg = make_cfg()
  for k, v in SIZES[tag].items():
    cfg[k] = v
  cfg.batch_size = N
  return cfg


def variable_shapes(tag):
  """[(TF variable name, shape)] of theta_g, theta_c, theta_v in the order checkpoint.tf_name_map lists them.  The
  recording script asserts that the reference's text creates exactly these; the CPU test holds export_tf_dict to the
  RECORDED list, not to this one."""
  s = SIZES[tag]
  size, base, fc1, dims = s['source_img_size'], s['base_channels'], s['fc1_size'], s['feature_extractor_dims']
  out = []

  def convs(prefix, cin, plan):
    for i, ch in enumerate(plan):
      name = prefix + ('Conv' if i == 0 else 'Conv_%d' % i)
      out.append((name + '/weights', (4, 4, cin, ch)))
      out.append((name + '/biases', (ch,)))
      cin = ch

  def fc(name, cin, cout):
    out.append((name + '/weights', (cin, cout)))
    out.append((name + '/biases', (cout,)))

  def extractor_plan():
    plan, ch, sz = [base], base, size // 2
    while sz > 4:
      ch = dims // 16 if sz == 8 else ch * 2
      sz //= 2
      plan.append(ch)
    return plan

  def critic_plan():
    plan, ch, sz = [base], base, size // 2
    while sz > 4:
      ch, sz = ch * 2, sz // 2
      plan.append(ch)
    return plan

  nstate = 3 + NUM_FILTERS
  convs('generator/', 3 + nstate, extractor_plan())
  for j, p in enumerate(FILTER_PARAMS):
    fc('generator/filter_%d/fc1' % j, dims, fc1)
    fc('generator/filter_%d/fc2' % j, fc1, p + 6)
  convs('generator/action_selection/', 3 + nstate, extractor_plan())
  fc('generator/action_selection/selector_fc1', dims, fc1)
  fc('generator/action_selection/selector_fc2', fc1, NUM_FILTERS)
  for scope, extra in (('critic/', 3), ('rl_value/critic/', nstate + 3)):
    plan = critic_plan()
    convs(scope, 3 + extra, plan)
    fc(scope + 'fully_connected', 16 * plan[-1], fc1)
    fc(scope + 'fully_connected_1', fc1, 1)
  return out


def weights(tag, seed=None, critic_fc2_scale=1.0):
  """{TF name: float64 array holding float32 values}: PCG64 normal draws in `variable_shapes` order, He-scaled kernels
  (sqrt(2 / fan_in)), biases of standard deviation 0.05, the critic's last layer times `critic_fc2_scale`."""
  rng = np.random.Generator(np.random.PCG64(SEEDS[tag] if seed is None else seed))
  out = {}
  for name, shape in variable_shapes(tag):
    a = rng.standard_normal(shape)
    if name.endswith('/biases'):
      a *= 0.05
    else:
      a *= np.sqrt(2.0 / np.prod(shape[:-1]))
    if name == 'critic/fully_connected_1/weights':
      a *= critic_fc2_scale
    out[name] = a.astype(np.float32).astype(np.float64)
  return out


def weights_sha256(w):
  h = hashlib.sha256()
  for name in sorted(w):
    h.update(name.encode())
    h.update(np.ascontiguousarray(w[name], dtype=np.float32).tobytes())
  return h.hexdigest()


def _images(rng, shape):
  """Multiples of 2^-10 in [-0.1, 1.25] (exact in fp16 and fp32) with the pixel classes of tests/test_hip_stats.py::
  stats_case in front of every image: grey, a two-way tie, exactly 1 and 0, max + min == 1."""
  lo, hi = -102, 1280  # codes: x = code / 1024
  code = rng.integers(lo, hi + 1, size=shape)
  # (two thirds of the pixels inside [0, 1]: the squares pull the draw towards the dark end, like linear RAW)
  inside = rng.random(shape[:-1]) < 0.67
  dark = (rng.random(shape)**2 * 1024).astype(np.int64)
  code = np.where(inside[..., None], dark, code)
  flat = code.reshape(shape[0], -1, 3)
  k = 4
  flat[:, 0:k] = flat[:, 0:k, :1]              # grey
  flat[:, k:2 * k, 1] = flat[:, k:2 * k, 0]    # two-way tie
  flat[:, 2 * k:3 * k, 2] = 1024               # exactly 1
  flat[:, 3 * k:4 * k, 0] = 0                  # exactly 0
  flat[:, 4 * k:5 * k] = np.array([768, 512, 256])  # max + min == 2 - max - min
  return flat.reshape(shape) / 1024.0


def inputs(tag, seed=None):
  """Every supplied input of K, L and G as float64 arrays whose values float32 holds exactly."""
  s = SIZES[tag]
  size, dims = s['source_img_size'], s['feature_extractor_dims']
  rng = np.random.Generator(np.random.PCG64((SEEDS[tag] if seed is None else seed) + 1000))
  f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)
  shape = (N, size, size, 3)
  out = dict(real_data=_images(rng, shape), fake_input=_images(rng, shape), fake_output=_images(rng, shape))
  states = np.zeros((N, 3 + NUM_FILTERS))
  states[:, 2] = STEPS
  states[:, 3:] = rng.random((N, NUM_FILTERS)) < 0.3
  out['states'] = states
  new_states = np.zeros((N, 3 + NUM_FILTERS))
  new_states[:, 0] = new_states[:, 1] = L_STOPPED
  new_states[:, 2] = L_STEPS
  new_states[:, 3:] = rng.random((N, NUM_FILTERS)) < 0.4
  out['new_states'] = new_states
  out['surrogate'] = f32(-2.0 - rng.random((N, 1)))     # log-probabilities near log(1 / 8)
  out['penalty'] = f32(rng.random((N, 1)) * 0.5)
  out['alpha'] = f32(np.round(rng.random((N, 1, 1, 1)) * 256) / 256)
  z = f32(rng.random((N, 3 + 16 * NUM_FILTERS)))
  z[:, 0] = SELECTION_NOISE
  out['z'] = z
  out['dropout_masks'] = (rng.random((2, N, dims)) < 0.5).astype(np.float64)
  out['logit_cotangent'] = f32(rng.standard_normal((N, 1)))  # K: c of sum(logit c)
  out['progress'] = np.array(PROGRESS)
  return out


def inputs_sha256(inp):
  h = hashlib.sha256()
  for name in sorted(inp):
    h.update(name.encode())
    h.update(np.ascontiguousarray(inp[name], dtype=np.float32).tobytes())
  return h.hexdigest()


def sample_stride(size):
  """The smallest prime above size / 8192: P stores a weight gradient at every k-th index of the flattened TF layout."""
  k = int(size // 8192) + 1
  while k < 2 or any(k % d == 0 for d in range(2, int(k**0.5) + 1)):
    k += 1
  return k
