"""GPU: ``Agent.curve_dispatch`` / ``GAN(..., curve_dispatch=True)`` at cfg.curve_steps 4 and 16 -- the agent's step on
the per-image dispatch for any step count -- against the float64 oracle and against the stack-and-select path it
replaces: losses, gradients, the high-resolution path, hipGraph capture and inference."""
import numpy as np
import pytest
import torch

from exposure_amd import checkpoint, evaluate
from exposure_amd.agent import Agent
from exposure_amd.config import make_cfg
from exposure_amd.gan import GAN
from oracle import filters_np as fnp
from oracle import nets_np as nn_np
from tests import _curve_dispatch_ref as C
from tests._tol import assert_image_close
from tests.test_oracle_nets import make_batch, spread_selection_noise

pytestmark = pytest.mark.gpu

# |a - b| <= R max|b| per agent parameter tensor, switch on against off: two fp32 evaluations of the same sums in different
# orders.  Measured on an MI355X: worst ratio 4.85e-7 (L = 4) and 3.46e-7 (L = 16); R = 8 x the worst, far below the 1e-3 cap
# (a missing term or a wrong head is O(1)).  DESIGN.md section 3.26 carries the same figures.
GRAD_RATIO_MEASURED = 4.85e-7
GRAD_RATIO = min(8 * GRAD_RATIO_MEASURED, 1e-3)


def gan_pair(steps, dev):
  """The same weights with the switch off and on, and a batch of 8 that selects every filter once."""
  cfg = make_cfg()
  cfg.curve_steps = steps
  gans = []
  for switch in (False, True):
    torch.manual_seed(1)
    gans.append(GAN(cfg, device=dev, curve_dispatch=switch))
  fake_input, real, states, z, masks, alpha = make_batch(8, 3)
  z = spread_selection_noise(gans[0], dev, fake_input, z, states, masks)
  return cfg, gans, (fake_input, real, states, z, masks)


@pytest.mark.parametrize('steps', [4, 16])
def test_generator_losses_and_gradients(steps, gpu_device):
  dev = gpu_device
  cfg, (off, on), (fake_input, real, states, z, masks) = gan_pair(steps, dev)
  t = lambda a: torch.from_numpy(a).to(dev)
  d = lambda a: a.astype(np.float64)
  ocfg = dict(nn_np.DEFAULT_CFG, curve_steps=steps)
  weights = {k: v.astype(np.float64) for k, v in checkpoint.export_tf_dict(on).items()}
  ref = nn_np.generator_losses(d(fake_input), d(z), d(states), 0.3, ocfg, weights, [d(m) for m in masks], 1)
  assert set(ref['debug']['selected_filter_id'].tolist()) >= {4, 7}, 'the batch must select both curve filters'
  grads = []
  for gan in (off, on):
    out = gan.generator_losses(t(fake_input), t(z), t(states), 0.3, 1, [t(m) for m in masks])
    assert ('params48' in out['debug']) and ('params24' not in out['debug'])
    assert np.array_equal(out['debug']['selected_filter_ids'].cpu().numpy(), ref['debug']['selected_filter_id'])
    err = np.abs(out['fake_output'].detach().float().cpu().numpy() - ref['fake_output'])
    assert (err <= 1e-3 + 1e-3 * np.abs(ref['fake_output'])).all(), err.max()
    for key in ('g_loss', 'v_loss'):
      assert abs(float(out[key].detach()) - ref[key]) <= 1e-4 * max(1.0, abs(ref[key])), key
    gan.zero_grad(set_to_none=True)
    (out['g_loss'] + out['v_loss']).backward()
    grads.append({k: p.grad.detach().clone() for k, p in gan.generator.named_parameters() if p.grad is not None})
    selected = out['debug']['selected_filter_ids']
  g_off, g_on = grads
  assert set(g_on) == set(g_off) == {k for k, _ in on.generator.named_parameters()}
  worst = 0.0
  for name, b in g_off.items():
    a = g_on[name]
    assert bool(torch.isfinite(a).all()), name
    scale = float(b.abs().max())
    ratio = float((a - b).abs().max()) / scale if scale > 0 else float((a - b).abs().max())
    worst = max(worst, ratio)
    assert ratio <= GRAD_RATIO, (name, ratio)
  print('L = %d: worst |on - off| / max|off| over the agent\'s parameter gradients: %.3e (bound %.1e)' % (steps, worst, GRAD_RATIO))
  # heads no image selected: exactly zero fc2 gradients (n = 8 selects every filter once; drop one and look again)
  keep = selected != 4
  idx = keep.nonzero().flatten()
  on.zero_grad(set_to_none=True)
  sub = on.generator_losses(t(fake_input)[idx], t(z)[idx], t(states)[idx], 0.3, 1, [t(m)[idx] for m in masks])
  assert 4 not in sub['debug']['selected_filter_ids'].tolist()
  (sub['g_loss'] + sub['v_loss']).backward()
  tone = on.generator.filters[4]
  assert float(tone.fc2.weight.grad.abs().max()) == 0 and float(tone.fc2.bias.grad.abs().max()) == 0
  assert float(on.generator.filters[7].fc2.weight.grad.abs().max()) > 0


@pytest.mark.parametrize('steps', [4, 16])
def test_high_res_path(steps, gpu_device):
  dev = gpu_device
  cfg = make_cfg()
  cfg.curve_steps = steps
  rng = np.random.default_rng(steps)
  low = torch.from_numpy((rng.random((2, 64, 64, 3))**2.2).astype(np.float16)).to(dev)
  high = torch.from_numpy((rng.random((2, 96, 128, 3))**2.2 * 1.3).astype(np.float16)).to(dev)
  states = torch.zeros((2, cfg.num_state_dim), device=dev)
  z = torch.from_numpy(rng.random((2, cfg.z_dim)).astype(np.float32)).to(dev)
  masks = [torch.from_numpy((rng.random((2, 4096)) < 0.5).astype(np.float32)).to(dev) for _ in range(2)]
  torch.manual_seed(2)
  agent = Agent(cfg).to(dev)
  # a selector that ignores its features: the bias alone picks the filter, first Tone, then Color
  with torch.no_grad():
    agent.selector_fc2.weight.zero_()
  seen = []
  for tone_or_color in (4, 7):
    with torch.no_grad():
      agent.selector_fc2.bias.zero_()
      agent.selector_fc2.bias[tone_or_color] = 9.0
    outs = {}
    for switch in (False, True):
      agent.curve_dispatch = switch
      with torch.no_grad():
        (out, new_states, hi), dbg, _ = agent((low, z, states), 0, 0.0, high_res=high, dropout_masks=masks)
      outs[switch] = (out, hi, dbg)
    (o0, h0, d0), (o1, h1, d1) = outs[False], outs[True]
    assert torch.equal(d0['selected_filter_ids'], d1['selected_filter_ids']) and torch.equal(d0['abi_filter_ids'], d1['abi_filter_ids'])
    ids = d1['abi_filter_ids'].cpu().numpy()
    assert (ids == tone_or_color).all()
    seen.append(tone_or_color)
    for hi_out, dbg in ((h0, d0), (h1, d1)):
      rows = dbg['params48'].cpu().numpy()
      for i, fid in enumerate(ids):
        p = C.num_params(int(fid), steps)
        ref = fnp.process_packed(int(fid), high[i:i + 1].cpu().numpy().astype(np.float64), rows[i:i + 1, :p].astype(np.float64))
        assert_image_close(hi_out[i:i + 1].float().cpu().numpy(), ref, np.float16, 'high_res_output L = %d filter %d' % (steps, fid))
    assert (d1['params48'][:, C.num_params(tone_or_color, steps):] == 0).all()
  assert seen == [4, 7]


def test_captured_iterations_train_bit_identically_to_eager_ones(gpu_device):
  """GAN(use_graphs=True, curve_dispatch=True) at 16 steps, two train_iterations at the training batch size, against the
  same GAN without graphs: every reported loss and a checksum of the agent's weights, bit for bit."""
  from exposure_amd.replay_memory import ReplayMemory, ResidentProvider
  dev = gpu_device
  cfg = make_cfg()
  cfg.curve_steps = 16
  cfg.replay_memory_size, cfg.citers = 2 * cfg.batch_size, 2
  runs = []
  for graphs in (True, False):
    torch.manual_seed(0)
    gan = GAN(cfg, device=dev, use_graphs=graphs, seed=4, curve_dispatch=True)
    mem = ReplayMemory(cfg, ResidentProvider(dev, dtype=torch.float16, seed=1, count=256),
                       ResidentProvider(dev, gamma=1.0, dtype=torch.float16, seed=2, count=192), seed=0)
    for _ in range(6):  # iteration 0's roll-out, shortened: terminated records for the critic
      feed, feats = mem.get_feed_dict_and_states(cfg.batch_size, lazy=True)
      g = gan.generator_step(feed['fake_input'], feed['z'], feed['states'], 0.0, it=0)
      mem.replace_memory(g['fake_output'], g['new_states'], feats, advanced=True)
    vals = []
    for it in (1, 2):
      out = gan.train_iteration(mem, it)
      vals += [out['g'][k].clone().reshape(-1)[:1] for k in ('g_loss', 'v_loss')] + [out['c']['c_loss'].clone().reshape(-1)[:1]]
    torch.cuda.synchronize()
    checksum = torch.stack([p.detach().double().sum() for p in gan.generator.parameters()])
    runs.append((torch.cat(vals), checksum))
  assert bool(torch.isfinite(runs[0][0]).all())
  assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
  assert torch.equal(runs[0][1], runs[1][1])


def test_inference_with_the_fused_chain(gpu_device):
  dev = gpu_device
  steps = 16
  cfg = make_cfg()
  cfg.curve_steps = steps
  torch.manual_seed(5)
  agent = Agent(cfg).to(dev)
  rng = np.random.default_rng(8)
  images = [torch.from_numpy((rng.random((h, w, 3))**2.2).astype(np.float16)).to(dev) for h, w in ((96, 128), (40, 72), (65, 33))]
  n = len(images)
  z = torch.from_numpy(rng.random((n, cfg.z_dim)).astype(np.float32)).to(dev)
  masks = [[torch.from_numpy((rng.random((n, 4096)) < 0.5).astype(np.float32)).to(dev) for _ in range(2)]
           for _ in range(cfg.test_steps)]
  res = {}
  for switch in (False, True):
    agent.curve_dispatch = switch
    res[switch] = evaluate.retouch_batch(agent, images, z=z, dropout_masks=masks, return_trace='full', curves='fused')
  (outs0, _l0, _s0, ops0), (outs1, _l1, _s1, ops1) = res[False], res[True]
  assert torch.equal(ops0['selected'], ops1['selected']) and torch.equal(ops0['abi_filter_ids'], ops1['abi_filter_ids'])
  for outs, ops in ((outs0, ops0), (outs1, ops1)):
    ids, rows = ops['abi_filter_ids'].cpu().numpy(), ops['params48'].cpu().numpy().astype(np.float64)
    for i, img in enumerate(images):
      cur = img.cpu().numpy().astype(np.float64)[None]
      for s in range(ids.shape[1]):
        fid = int(ids[i, s])
        cur = fnp.process_packed(fid, cur, rows[i:i + 1, s, :C.num_params(fid, steps)]) if fid >= 0 else cur * 0
      assert_image_close(outs[i].float().cpu().numpy()[None], cur, np.float16, 'retouch_batch image %d' % i)
