"""CPU: the 16-bit pictures of evaluate.retouch / retouch_batch (picture='u16', intermediates='u16') and of the CLI's
--tiff16, with the C-ABI binding mocked by the oracle (tests/_fake_hip.py) and stand-ins for the three tap calls defined
here by what the kernels promise: storage tap k is the running image after step k rounded to the storage dtype, the
u8 tap save_png's encoding of it, the u16 tap clip(rint(float32(s) * 65535), 0, 65535).  Also encode_u16 against that
definition and the TIFF writer the CLI now uses.  The GPU counterpart is tests/test_hip_chain_taps16.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import evaluate, tiff16
from exposure_amd.config import make_cfg
from oracle import filters_torch as ft
from tests import _fake_hip
from tests._fake_hip import fake_hip
from tests.test_masked_chain_host import masked_agent
from tests.test_taps_host import _ragged_fwd, _truncated, agent, host_u8, images, inputs


def host_u16(a):
  """the definition of EXPO_TAP_U16 / encode_u16 on a float array"""
  return np.clip(np.rint(np.asarray(a).astype(np.float32) * np.float32(65535)), 0, 65535).astype(np.uint16)


def u16(t):
  """a uint16 tensor as a NumPy array"""
  assert t.dtype == torch.uint16
  return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _put(tap, s):
  """write the storage values s into one tap plane of any of the three formats"""
  if tap.dtype == torch.uint16:
    tap.view(torch.int16).copy_(torch.from_numpy(host_u16(s.float().numpy()).view(np.int16)))
  elif tap.dtype == torch.uint8:
    tap.copy_(torch.from_numpy(host_u8(s.float().numpy())))
  else:
    tap.copy_(s)


calls = []  # (entry point, number of images, tap dtype) of every tap call


def _taps_fwd(ids, params, x, y, tap_mask, taps, name='dense'):
  if name:
    calls.append((name, x.shape[0], None if taps is None else taps.dtype))
  if y is not None:
    _fake_hip._chain_fused_fwd(ids, params, x, y)
  j = 0
  for k in range(ids.shape[1]):
    if (tap_mask >> k) & 1:
      _put(taps[j], _truncated(ids, params, x, k))
      j += 1
  assert taps is None or j == taps.shape[0]


def _ragged_taps_fwd(ids, params, xs, ys, tap_mask, taps):
  calls.append(('ragged', len(xs), None if taps is None else taps[0].dtype))
  for i, x in enumerate(xs):
    x4 = x if x.dim() == 4 else x[None]
    y4 = None if ys is None else ys[i].reshape(x4.shape)
    _taps_fwd(ids[i:i + 1], params[i:i + 1], x4, y4, tap_mask, None if taps is None else taps[i][:, None], name=None)


def _masked_ragged(ids, params, mask_params, xs, ys, maximum_sharpness, minimum_strength, tap_mask=0, taps=None):
  calls.append(('masked', len(xs), None if taps is None else taps[0].dtype))
  for i, x in enumerate(xs):
    cur = x.reshape(1, *x.shape[-3:]).double()
    j = 0
    for k in range(ids.shape[1]):
      fid = int(ids[i, k])
      if fid < 0:
        cur = torch.zeros_like(cur)
      else:
        cur = ft.apply_masked(fid, cur, params[i:i + 1, k, :_fake_hip.NUM_PARAMS[fid]].double(),
                              _fake_hip._raw_mask(mask_params[i:i + 1, k]), maximum_sharpness, minimum_strength)
      if (tap_mask >> k) & 1:
        _put(taps[i][j], cur[0].to(x.dtype))
        j += 1
    if ys is not None:
      ys[i].copy_(cur.reshape(x.shape).to(x.dtype))


@contextlib.contextmanager
def fake_taps16():
  with fake_hip(), mock.patch.multiple('exposure_amd._cabi', chain_fused_fwd_ragged=_ragged_fwd,
                                       chain_fused_fwd_taps=_taps_fwd, chain_fused_fwd_ragged_taps=_ragged_taps_fwd,
                                       chain_fused_masked_fwd_ragged=_masked_ragged):
    yield


def test_encode_u16_is_the_numpy_definition():
  ties = (np.arange(65536, dtype=np.float64) + 0.5) / 65535.0
  v = np.concatenate([ties, np.linspace(-2, 3, 4001), [0.0, -0.0, 1.0, 65504.0, -65504.0, np.inf, -np.inf]])
  v = np.concatenate([v, np.zeros(-len(v) % 3)]).astype(np.float32).reshape(-1, 3)
  got = evaluate.encode_u16(torch.from_numpy(v))
  assert got.dtype == torch.uint16 and got.shape == v.shape and got.is_contiguous()
  np.testing.assert_array_equal(u16(got), host_u16(v))
  assert u16(got).min() == 0 and u16(got).max() == 65535
  # a strided input, and fp16 storage: the fp16 value is what gets encoded
  h = torch.from_numpy(v[:3000].astype(np.float16).reshape(10, 100, 3, 3)).transpose(0, 1)
  np.testing.assert_array_equal(u16(evaluate.encode_u16(h)), host_u16(h.numpy()))
  # every code is reached from its own centre
  c = np.arange(65536, dtype=np.float32) / np.float32(65535)
  c = c.reshape(-1, 4)
  assert u16(evaluate.encode_u16(torch.from_numpy(c))).reshape(-1).tolist() == list(range(65536))


def test_write_tiff_round_trips_an_odd_width(tmp_path):
  rng = np.random.default_rng(2)
  a = rng.integers(0, 65536, (7, 13, 3), dtype=np.uint16)
  a[0, 0], a[-1, -1] = (0, 65535, 0x1234), (0xFF00, 0x00FF, 1)
  p = str(tmp_path / 'a.tif')
  assert evaluate.save_tiff_u16(p, a) == p
  b = tiff16.read_tiff(p)
  assert b.dtype == np.uint16 and b.shape == a.shape
  np.testing.assert_array_equal(b, a)
  raw = open(p, 'rb').read()
  assert raw[:2] == b'II' and raw[8:8 + a.size * 2] == a.astype('<u2').tobytes()  # the strip is the array byte for byte


def _same_run(a, b):
  """output, proxies, states and the trace of two retouch / retouch_batch results are bit-equal"""
  outs_a, outs_b = (a[0], b[0]) if isinstance(a[0], list) else ([a[0]], [b[0]])
  assert all(torch.equal(u, v) for u, v in zip(outs_a, outs_b))
  assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
  for k in b[3]:
    assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize('masking', [False, True])
def test_retouch_u16_pictures_and_intermediates(masking):
  if masking:
    cfg, ag = masked_agent()
  else:
    cfg = make_cfg()
    ag = agent(cfg)
  hi = torch.cat(images([(24, 40)] * 2, 1))
  z, masks = inputs(cfg, 2, 2)
  kw = dict(z=z, dropout_masks=masks, return_trace='full', masks='fused')
  del calls[:]
  with fake_taps16():
    ref = evaluate.retouch(ag, hi, **kw)
    st = evaluate.retouch(ag, hi, intermediates='storage', **kw)
    n_before = len(calls)
    pic = evaluate.retouch(ag, hi, picture='u16', **kw)
    inter = evaluate.retouch(ag, hi, intermediates='u16', **kw)
    both = evaluate.retouch(ag, hi, picture='u16', intermediates='u16', **kw)
    mixed = evaluate.retouch(ag, hi, picture='u16', intermediates='storage', **kw)
    step = evaluate.retouch(ag, hi, picture='u16', intermediates='u16', fused=False, **kw)
  # one launch each, with uint16 taps (the storage mix: storage taps, the picture encoded from the output)
  name = 'masked' if masking else 'dense'
  assert calls[n_before:] == [(name, 2, torch.uint16)] * 3 + [(name, 2, torch.float32)]
  for r, extra in ((pic, 1), (inter, 1), (both, 2), (mixed, 2)):
    assert len(r) == 4 + extra
    _same_run(r, ref)
  want_pic = host_u16(ref[0].numpy())
  for r in (pic, both, mixed):
    assert r[-1].dtype == torch.uint16 and r[-1].shape == hi.shape
    np.testing.assert_array_equal(u16(r[-1]), want_pic)
    np.testing.assert_array_equal(u16(r[-1]), u16(evaluate.encode_u16(ref[0])))
  for r in (inter, both):
    assert r[4].dtype == torch.uint16 and r[4].shape == (cfg.test_steps - 1, 2, 24, 40, 3)
    np.testing.assert_array_equal(u16(r[4]), host_u16(st[4].numpy()))
  assert torch.equal(mixed[4], st[4])
  # the reference's schedule: encode_u16 of the per-step tensors and of the output
  assert step[4].dtype == step[5].dtype == torch.uint16
  np.testing.assert_array_equal(u16(step[5]), host_u16(step[0].numpy()))
  # fp32 storage between steps moves a value by ~2^-24 relative, 0.004 codes: at most one code at a rounding boundary
  assert int((step[4].int() - both[4].int()).abs().max()) <= 1


def test_u8_and_u16_do_not_mix_and_u8_is_unchanged():
  cfg = make_cfg()
  ag = agent(cfg)
  imgs = images([(16, 24), (9, 7)], 3)
  z, masks = inputs(cfg, 2, 4)
  with fake_taps16():
    for pic, inter in (('u16', 'u8'), ('u8', 'u16'), (True, 'u16')):
      with pytest.raises(ValueError):
        evaluate.retouch(ag, imgs[0], picture=pic, intermediates=inter)
      with pytest.raises(ValueError):
        evaluate.retouch_batch(ag, imgs, picture=pic, intermediates=inter)
    with pytest.raises(ValueError):
      evaluate.retouch(ag, imgs[0], picture='u32')
    with pytest.raises(ValueError):
      evaluate.retouch_batch(ag, imgs, picture='storage')
    a = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, picture=True, intermediates='u8')
    b = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, picture='u8', intermediates='u8')
  assert len(a) == len(b) == 5
  for u, v in zip(a[3] + a[4], b[3] + b[4]):
    assert u.dtype == torch.uint8 and torch.equal(u, v)
  assert 'u16' in evaluate.INTERMEDIATES


@pytest.mark.parametrize('masking', [False, True])
def test_retouch_batch_u16_pictures_and_intermediates(masking):
  if masking:
    cfg, ag = masked_agent()
  else:
    cfg = make_cfg()
    ag = agent(cfg)
  sizes = [(40, 56), (23, 17), (64, 48)]
  imgs = images(sizes, 7)
  imgs[1] = imgs[1][0]
  z, masks = inputs(cfg, 3, 8)
  kw = dict(z=z, dropout_masks=masks, return_trace='full', masks='fused')
  del calls[:]
  with fake_taps16():
    ref = evaluate.retouch_batch(ag, imgs, **kw)
    st = evaluate.retouch_batch(ag, imgs, intermediates='storage', **kw)
    n_before = len(calls)
    pic = evaluate.retouch_batch(ag, imgs, picture='u16', **kw)
    inter = evaluate.retouch_batch(ag, imgs, intermediates='u16', **kw)
    both = evaluate.retouch_batch(ag, imgs, picture='u16', intermediates='u16', **kw)
    mixed = evaluate.retouch_batch(ag, imgs, picture='u16', intermediates='storage', **kw)
  name = 'masked' if masking else 'ragged'
  assert calls[n_before:] == [(name, 3, torch.uint16)] * 3 + [(name, 3, torch.float32)]  # one ragged launch per call
  for r in (pic, inter, both, mixed):
    _same_run(r, ref)
  for r in (pic, both, mixed):
    assert [tuple(t.shape) for t in r[-1]] == [(h, w, 3) for h, w in sizes]
    for t, o in zip(r[-1], ref[0]):
      np.testing.assert_array_equal(u16(t), host_u16(o.reshape(o.shape[-3:]).numpy()))
      np.testing.assert_array_equal(u16(t), u16(evaluate.encode_u16(o.reshape(o.shape[-3:]))))
  for r in (inter, both):
    assert [tuple(t.shape) for t in r[4]] == [(cfg.test_steps - 1, h, w, 3) for h, w in sizes]
    for t, s in zip(r[4], st[4]):
      np.testing.assert_array_equal(u16(t), host_u16(s.numpy()))


def test_retouch_batch_generic_curves_fall_back_to_encode_u16():
  cfg = make_cfg()
  cfg.curve_steps = 4
  ag = agent(cfg)
  imgs = images([(24, 40), (33, 21)], 9)
  z, masks = inputs(cfg, 2, 10)
  del calls[:]
  with fake_taps16():
    outs, _, _, inter, pics = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, intermediates='u16',
                                                     picture='u16')
    _, _, _, st = evaluate.retouch_batch(ag, imgs, z=z, dropout_masks=masks, intermediates='storage')
  assert calls == []  # the reference's schedule on the generic kernels: no tap call
  for o, t, s, p in zip(outs, inter, st, pics):
    np.testing.assert_array_equal(u16(t), host_u16(s.numpy()))
    np.testing.assert_array_equal(u16(p), host_u16(o[0].numpy()))


def _write_tiffs(tmp_path, sizes):
  rng = np.random.default_rng(11)
  paths = []
  for i, (h, w) in enumerate(sizes):
    p = str(tmp_path / ('in%d.tif' % i))
    tiff16.write_tiff(p, (rng.random((h, w, 3))**1.5 * 60000).astype(np.uint16))
    paths.append(p)
  return paths


@pytest.mark.parametrize('mode', [['--batch', '3'], ['--batch', '1'], ['--stepwise'], ['--batch', '3', '--masking',
                                                                                         '--fused-masks']])
def test_cli_tiff16_files_and_records(tmp_path, mode):
  sizes = [(20, 30), (17, 9), (32, 32)]
  paths = _write_tiffs(tmp_path, sizes)
  out = str(tmp_path / 'out') + os.sep
  del calls[:]
  with fake_taps16(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    recs = evaluate.main(['--seed', '3', '--dtype', 'f32', '--tiff16', '--step-by-step', '--out', out, *mode, *paths])
  assert len(recs) == 3
  if '--stepwise' in mode:
    assert calls == []
  elif mode[:2] == ['--batch', '3']:
    assert calls == [('masked' if '--masking' in mode else 'ragged', 3, torch.uint16)]  # output, picture, intermediates
  else:
    assert calls == [('dense', 1, torch.uint16)] * 3
  keys = ['intermediate%02d' % i for i in range(4)]
  for rec, p, (h, w) in zip(recs, paths, sizes):
    stem = os.path.join(out, os.path.basename(p)) + '.retouched'
    assert rec['png'] == {} and sorted(rec['tiff']) == sorted(['retouched'] + keys)
    assert rec['tiff']['retouched'] == stem + '.tif'
    for k in keys:
      assert rec['tiff'][k] == '%s.%s.tif' % (stem, k)
    for f in rec['tiff'].values():
      a = tiff16.read_tiff(f)
      assert a.dtype == np.uint16 and a.shape == (h, w, 3)
    # the retouched file is the encoding of the .npy output (fp32 storage: the file's own values)
    np.testing.assert_array_equal(tiff16.read_tiff(rec['tiff']['retouched']), host_u16(np.load(rec['output'])))
  assert not [f for f in os.listdir(out) if f.endswith('.png')]  # --step-by-step does not imply --png here
  assert len([f for f in os.listdir(out) if f.endswith('.tif')]) == 15
  if '--masking' not in mode:  # each intermediate is the replayed truncated chain of the record's own sequence
    rec = recs[0]
    x = torch.from_numpy(np.ascontiguousarray(evaluate.load_image(paths[0]))).float()[None]
    ids = torch.tensor([rec['abi_filter_ids']], dtype=torch.int32)
    prm = torch.from_numpy(rec['params24'])[None].float()
    for k in range(4):
      want = host_u16(_truncated(ids, prm, x, k)[0].numpy()).astype(int)
      got = tiff16.read_tiff(rec['tiff']['intermediate%02d' % k]).astype(int)
      assert int(np.abs(got - want).max()) <= (1 if mode == ['--stepwise'] else 0), k  # (stepwise: fp32 storage between steps)


def test_cli_tiff16_without_step_by_step_and_with_show_input(tmp_path):
  paths = _write_tiffs(tmp_path, [(12, 20)])
  out = str(tmp_path / 'o') + os.sep
  with fake_taps16(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    rec, = evaluate.main(['--seed', '5', '--dtype', 'f32', '--tiff16', '--show-input', '--out', out, *paths])
  assert sorted(rec['tiff']) == ['retouched'] and sorted(rec['png']) == ['input_tone_mapped']
  assert sorted(f.split('.', 2)[2] for f in os.listdir(out)) == ['retouched.input_tone_mapped.png', 'retouched.npy',
                                                                 'retouched.tif']
  np.testing.assert_array_equal(tiff16.read_tiff(rec['tiff']['retouched']), host_u16(np.load(rec['output'])))


@pytest.mark.parametrize('flags', [['--png'], ['--device-png'], ['--score', 'targets']])
def test_cli_tiff16_rejects_the_8_bit_outputs(tmp_path, flags, capsys):
  paths = _write_tiffs(tmp_path, [(8, 8)])
  with fake_taps16(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    with pytest.raises(SystemExit) as e:
      evaluate.main(['--tiff16', *flags, *paths])
  assert e.value.code == 2 and '--tiff16' in capsys.readouterr().err
  assert os.listdir(str(tmp_path)) == ['in0.tif']


def test_binding_maps_uint16_taps_to_format_3():
  from exposure_amd import _cabi
  assert _cabi._tap_format(torch.empty(1, dtype=torch.uint16), torch.float16) == _cabi.EXPO_TAP_U16 == 3
  assert _cabi._tap_format(torch.empty(1, dtype=torch.uint8), torch.float16) == _cabi.EXPO_TAP_U8
  assert _cabi._tap_format(torch.empty(1, dtype=torch.float32), torch.float32) == _cabi.EXPO_TAP_STORAGE
  with pytest.raises(_cabi.ExposureHipError, match='uint8, uint16 or'):
    _cabi._tap_format(torch.empty(1, dtype=torch.int16), torch.float16)
