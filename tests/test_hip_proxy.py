"""GPU: the agent's proxies on the device: expo_bilinear_resize_ragged against its NumPy restatement
bit for bit, against evaluate.make_low_res within the derived bound (tests/_bilinear_ref.py::parity_bound),
retouch_batch(proxy='device', picture=True) against fused_chain_ragged on its own trace, and the CLI's --device-proxy
--device-png against --png.  The host half is tests/test_proxy_host.py."""
import os

import numpy as np
import pytest
import torch

from exposure_amd import _cabi, evaluate
from exposure_amd.agent import Agent
from exposure_amd.config import make_cfg
from tests import _bilinear_ref as br

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
S = 64
NP = {torch.float16: np.float16, torch.float32: np.float32}
DTYPES = [(torch.float16, torch.float16), (torch.float32, torch.float32), (torch.float16, torch.float32)]
SIZES = [(1, 1), (63, 65), (64, 64), (513, 769), (6000, 4000), (40, 23), (97, 131)]


def photo(rng, h, w, dtype):
  return torch.from_numpy(rng.random((h, w, 3), dtype=np.float32)**2.2 * 1.6).to(dtype)


def same_bits(a, b):
  assert a.dtype == b.dtype and a.shape == b.shape
  it = torch.int16 if a.dtype == torch.float16 else torch.int32
  bad = a.contiguous().view(it) != b.contiguous().view(it)
  assert not bool(bad.any()), '%d of %d values differ' % (int(bad.sum()), bad.numel())


def make_case(rng, in_dtype):
  """One image per size (host copies kept), the last but one behind a base pointer offset by one pixel; windows: every
  centre, windows that are not the centre (odd offsets, sides below and above S), and enough more that the call holds
  65 windows (two launches)."""
  hosts = [photo(rng, h, w, in_dtype) for h, w in SIZES]
  xs = [a.to(DEV) for a in hosts]
  h, w = SIZES[-1]
  buf = torch.empty(h * w * 3 + 3, dtype=in_dtype, device=DEV)
  buf[3:].copy_(xs[-1].reshape(-1))
  xs[-1] = buf[3:].view(h, w, 3)  # contiguous, its first element one pixel into the allocation
  assert xs[-1].data_ptr() == buf.data_ptr() + 3 * buf.element_size() and xs[-1].is_contiguous()
  wins = evaluate.center_windows(SIZES)
  wins += [(3, 7, 11, 500), (3, 1, 257, 511), (3, 450, 700, 63), (4, 1999, 1, 3999), (4, 5, 3, 17), (1, 2, 1, 61),
           (6, 1, 3, 64), (6, 33, 67, 64), (0, 0, 0, 1)]
  k = 0
  while len(wins) < 65:
    wins.append((6, (7 * k) % 30, (11 * k + 1) % 60, 67 - (k % 5) * 9))
    k += 1
  return xs, hosts, wins


def reference(hosts, wins, out_dtype):
  return torch.from_numpy(np.stack([br.bilinear_resize(hosts[i].numpy()[y0:y0 + s, x0:x0 + s], S, NP[out_dtype])
                                    for i, y0, x0, s in wins]))


def resize(xs, wins, out_dtype):
  """One call into the middle of a guarded buffer; the guard rows must come back untouched."""
  buf = torch.full((len(wins) + 2, S, S, 3), 7.0, dtype=out_dtype, device=DEV)
  _cabi.bilinear_resize_ragged(xs, wins, S, buf[1:-1])
  torch.cuda.synchronize()
  assert bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all()), 'a write outside the output'
  return buf[1:-1].clone()


@pytest.mark.parametrize('in_dtype,out_dtype', DTYPES)
def test_kernel_equals_the_restatement_bit_for_bit(in_dtype, out_dtype):
  rng = np.random.default_rng(5 + DTYPES.index((in_dtype, out_dtype)))
  xs, hosts, wins = make_case(rng, in_dtype)
  assert len(wins) == 65
  got = resize(xs, wins, out_dtype)
  same_bits(got.cpu(), reference(hosts, wins, out_dtype))
  # side == S is the identity up to the cast
  i, y0, x0, s = wins[2]
  assert s == S and torch.equal(got[2], xs[i][y0:y0 + s, x0:x0 + s].to(out_dtype))
  # two runs; and every window alone against the same window inside the batch
  same_bits(resize(xs, wins, out_dtype), got)
  for k, win in enumerate(wins):
    one = resize([xs[win[0]]], [(0,) + tuple(win[1:])], out_dtype)
    assert torch.equal(one[0], got[k]), (k, win)


def test_other_output_sizes_and_a_one_by_one_output():
  rng = np.random.default_rng(9)
  hosts = [photo(rng, 150, 101, torch.float32), photo(rng, 9, 20, torch.float32)]
  xs = [a.to(DEV) for a in hosts]
  for s_out in (1, 7, 80, 256):
    wins = [(0, 3, 0, 101), (1, 0, 2, 9), (0, 40, 30, 1)]
    out = torch.empty((len(wins), s_out, s_out, 3), dtype=torch.float32, device=DEV)
    _cabi.bilinear_resize_ragged(xs, wins, s_out, out)
    want = np.stack([br.bilinear_resize(hosts[i].numpy()[y0:y0 + s, x0:x0 + s], s_out) for i, y0, x0, s in wins])
    same_bits(out.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_kernel_within_the_derived_bound_of_make_low_res(dtype):
  """torch's kernel may contract the coordinate: the values agree within parity_bound, in fp32 storage as well, so that
  the fp16 ulp cannot hide an error.  Prints the observed worst difference and the count of differing values."""
  rng = np.random.default_rng(31)
  worst, differ, total = 0.0, 0, 0
  for h, w in SIZES:
    host = photo(rng, h, w, dtype)
    x = host.to(DEV)
    got = evaluate.make_low_res_batch([x], S)[0]
    want = evaluate.make_low_res(x[None], S)[0]
    assert got.dtype == want.dtype == dtype
    (_, y0, x0, side), = evaluate.center_windows([(h, w)])
    bound = br.parity_bound(host.numpy()[y0:y0 + side, x0:x0 + side], S, NP[dtype])
    err = (got.double() - want.double()).abs().cpu().numpy()
    worst, differ, total = max(worst, float(err.max())), differ + int((err > 0).sum()), total + err.size
    print('proxy parity %s %dx%d: worst |device - make_low_res| %.3g, %d of %d values differ, smallest margin %.3g'
          % (NP[dtype].__name__, h, w, err.max(), int((err > 0).sum()), err.size, (bound - err).min()))
    assert (err <= bound).all(), (h, w, float(err.max()))
  print('proxy parity %s total: worst %.3g, %d of %d values differ' % (NP[dtype].__name__, worst, differ, total))


def _agent(cfg, seed=4):
  torch.manual_seed(seed)
  return Agent(cfg).to(DEV)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_retouch_batch_device_proxy_and_pictures(dtype):
  cfg = make_cfg()
  ag = _agent(cfg)
  rng = np.random.default_rng(41)
  sizes = [(301, 450), (64, 64), (777, 512), (40, 23), (1200, 1600)]
  imgs = [photo(rng, h, w, dtype).to(DEV) for h, w in sizes]
  imgs[1] = imgs[1][None]
  g = torch.Generator().manual_seed(42)
  z = torch.rand(len(sizes), cfg.z_dim, generator=g).to(DEV)
  masks = [[(torch.rand(len(sizes), 4096, generator=g) < 0.5).float().to(DEV) for _ in range(2)]
           for _ in range(cfg.test_steps)]
  outs, low, states, ops, pics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full',
                                                        proxy='device', picture=True)
  # low, states and trace are what the agent makes of make_low_res_batch's proxies
  wlow, wstates, _, wtrace, wids, wprm, _, _ = evaluate._agent_steps(ag, evaluate.make_low_res_batch(imgs, S), z,
                                                                     cfg.test_steps, masks)
  assert torch.equal(low, wlow) and torch.equal(states, wstates) and torch.equal(ops['selected'], torch.stack(wtrace, dim=1))
  assert torch.equal(ops['abi_filter_ids'], torch.stack(wids, dim=1)) and torch.equal(ops['params24'], torch.stack(wprm, dim=1))
  replay = evaluate.fused_chain_ragged(imgs, ops['abi_filter_ids'], ops['params24'])
  for o, r, p, im in zip(outs, replay, pics, imgs):
    assert o.shape == im.shape and torch.equal(o, r)
    assert p.dtype == torch.uint8 and p.shape == im.shape[-3:]
    assert torch.equal(p, evaluate.encode_u8(o).reshape(p.shape))
  # with u8 intermediates the pictures come from the same launch and nothing else changes
  res = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full', proxy='device',
                               intermediates='u8', picture=True)
  ref = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, return_trace='full', proxy='device',
                               intermediates='u8')
  for i in range(len(sizes)):
    assert torch.equal(res[0][i], outs[i]) and torch.equal(res[5][i], pics[i]) and torch.equal(res[4][i], ref[4][i])
  # retouch on one image: the same proxy, picture = the encoded output
  one = evaluate.retouch(ag, imgs[0][None], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], proxy='device',
                         picture=True)
  assert torch.equal(one[3], evaluate.encode_u8(one[0]))
  step = evaluate.retouch(ag, imgs[0][None], z=z[:1], dropout_masks=[[m[:1] for m in s] for s in masks], proxy='device',
                          picture=True, fused=False)
  assert torch.equal(step[3], evaluate.encode_u8(step[0]))


@pytest.mark.parametrize('mode', [['--batch', '4'], ['--batch', '1'], ['--stepwise']])
def test_cli_device_proxy_device_png_equal_png(tmp_path, mode):
  from PIL import Image
  rng = np.random.default_rng(51)
  paths = []
  for i, (h, w) in enumerate([(40, 56), (333, 210), (64, 48), (500, 700), (90, 90)]):
    p = str(tmp_path / ('in%d.png' % i))
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 'RGB').save(p)
    paths.append(p)
  runs = []
  for flag in ('--device-png', '--png'):
    out = str(tmp_path / flag.strip('-')) + os.sep
    runs.append(evaluate.main(['--seed', '3', '--device-proxy', flag, '--show-input', '--out', out, *mode, *paths]))
  dev, host = runs
  assert len(dev) == len(host) == len(paths)
  for a, b in zip(dev, host):
    assert a['filters'] == b['filters'] and a['abi_filter_ids'] == b['abi_filter_ids']
    assert open(a['output'], 'rb').read() == open(b['output'], 'rb').read()
    assert sorted(a['png']) == sorted(b['png']) == ['input_tone_mapped', 'retouched']
    for k in a['png']:
      np.testing.assert_array_equal(np.asarray(Image.open(a['png'][k])), np.asarray(Image.open(b['png'][k])), err_msg=k)
