"""CPU: the host half of the input pictures from integer codes -- evaluate.input_luts against the host
pictures (save_png's encoding of the decoded input and of tone_mapped_input of it) on random images of every decode kind
and storage dtype, its all-zero rule, and the routing of evaluate.input_pictures_raw and of the CLI's --show-linear /
--device-input-png, against CPU stand-ins of codes_max_ragged and codes_lut_ragged defined here by what
include/exposure_hip.h promises.  The decode runs on the stand-ins of tests/test_fused_decode_host.py.  The GPU
counterpart is tests/test_hip_input_pictures.py."""
import contextlib
import os
from unittest import mock

import numpy as np
import pytest
import torch

from exposure_amd import evaluate
from tests import test_fused_decode_host as fd

calls = []  # (entry point, number of images) of every call of a stand-in


def fake_codes_max(codes, workspace=None):
  calls.append(('max', len(codes)))
  return torch.tensor([int(fd._c3(c).max()) for c in codes], dtype=torch.int32)


def fake_codes_lut(codes, luts, stride, outs):
  calls.append(('lut', len(codes)))
  entries = 256 if codes[0].dtype is torch.uint8 else 65536
  assert stride == 0 or stride >= entries
  flat = luts.reshape(-1).numpy()
  for i, (c, o) in enumerate(zip(codes, outs)):
    o.copy_(torch.from_numpy(flat[i * stride + fd._c3(c)]))


@contextlib.contextmanager
def stand_ins():
  with fd.stand_ins(), mock.patch.multiple('exposure_amd._cabi', codes_max_ragged=fake_codes_max,
                                           codes_lut_ragged=fake_codes_lut):
    yield


def encode(a):
  """save_png's encoding"""
  return np.clip(np.rint(np.asarray(a, dtype=np.float32) * 255.0), 0, 255).astype(np.uint8)


def random_raws(seed):
  rng = np.random.default_rng(seed)
  raws = []
  for kind, ct, hi in (('srgb8', np.uint8, 256), ('srgb16', np.uint16, 65536), ('prophoto16', np.uint16, 65536)):
    for c in (1, 3, 4):
      top = int(rng.integers(hi // 8, hi))  # the largest code differs from image to image
      raws.append((rng.integers(0, top, (37, 53, c)).astype(ct), kind))
  return raws


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32])
def test_input_luts_gathered_by_code_are_the_host_pictures(dtype):
  """the check DESIGN.md §3.24 rests on: the project's expressions evaluated on the 256 / 65536 table values and
  gathered by code equal the same expressions evaluated on the whole decoded image, in every value -- so NumPy's pow
  gives a value the same result at any position of any array"""
  raws = random_raws(3)
  with stand_ins():
    images = evaluate.decode_images(raws, dtype, 'cpu')
    for (codes, kind), im in zip(raws, images):
      cs = [torch.from_numpy(codes)]
      tables, stride = fd.fake_decode_tables(cs, evaluate.decode_table(kind, 'cpu'), evaluate.DECODE_NORMALIZE[kind], dtype)
      lin, tone = evaluate.input_luts(tables, stride, fake_codes_max(cs))
      a = im[0].float().numpy()
      idx = fd._c3(cs[0])
      assert lin.dtype == np.uint8 and lin.shape == (1, tables.shape[1])
      assert np.array_equal(lin[0][idx], encode(a)), (kind, codes.shape[2])
      assert np.array_equal(tone[0][idx], encode(evaluate.tone_mapped_input(a))), (kind, codes.shape[2])
      lin16, tone16 = evaluate.input_luts(tables, stride, fake_codes_max(cs), 'u16')
      assert lin16.dtype == np.uint16
      assert np.array_equal(lin16[0][idx], evaluate._host_codes(evaluate.encode_u16(im[0])))
      t = torch.from_numpy(evaluate.tone_mapped_input(a))
      assert np.array_equal(tone16[0][idx], evaluate._host_codes(evaluate.encode_u16(t)))


def test_input_luts_rows_follow_the_stride_and_the_maxima():
  t = evaluate.decode_table('prophoto16', 'cpu')[None].to(torch.float16)  # one shared table, stride 0
  lin, tone = evaluate.input_luts(t, 0, torch.tensor([65535, 1000, 40000], dtype=torch.int32))
  assert lin.shape == tone.shape == (3, 65536)
  assert np.array_equal(lin[0], lin[1]) and np.array_equal(lin[0], lin[2])
  assert tone[0][65535] == 255 and tone[1][1000] == 255 and tone[2][40000] == 255
  assert tone[1][999] <= 255 and tone[1][65535] == 255  # beyond the maximum: saturated
  assert not np.array_equal(tone[0], tone[1])


@pytest.mark.parametrize('code', ['u8', 'u16'])
def test_all_zero_images_get_tables_of_zero(code):
  """the divisor t[m] is 0 (one shared table) or NaN (a normalised table of an all-zero image): tables of 0, where the
  reference divides by zero"""
  zero = torch.zeros((5, 7, 3), dtype=torch.uint8)
  live = torch.full((5, 7, 3), 9, dtype=torch.uint8)
  tables, stride = fd.fake_decode_tables([live, zero], evaluate.decode_table('srgb8', 'cpu'), 1, torch.float32)
  assert torch.isnan(tables[1]).all()
  with np.errstate(all='raise'):
    lin, tone = evaluate.input_luts(tables, stride, torch.tensor([9, 0], dtype=torch.int32), code)
  assert not lin[1].any() and not tone[1].any() and lin[0].any() and tone[0].any()
  shared = evaluate.decode_table('prophoto16', 'cpu')[None]
  lin, tone = evaluate.input_luts(shared, 0, torch.tensor([0], dtype=torch.int32), code)
  assert not lin.any() and not tone.any()


def test_input_pictures_raw_groups_order_and_values():
  raws = fd.mixed_raws(5)
  with stand_ins():
    images = evaluate.decode_images(raws, torch.float16, 'cpu')
    del calls[:]
    lin, tone = evaluate.input_pictures_raw(raws, torch.float16, 'cpu')
    made = list(calls)
    only, = evaluate.input_pictures_raw(raws, torch.float16, 'cpu', linear=False)
    staged = list(evaluate.stage_raws(raws, torch.float16, 'cpu'))
    del fd.calls[:]
    again = evaluate.input_pictures_raw(raws, torch.float16, 'cpu', staged=staged)
    assert not fd.calls  # staged: no second upload-and-tables pass
    with pytest.raises(ValueError, match='nothing requested'):
      evaluate.input_pictures_raw(raws, torch.float16, 'cpu', linear=False, tone_mapped=False)
    with pytest.raises(ValueError, match='no images'):
      evaluate.input_pictures_raw([], torch.float16, 'cpu')
  # per (kind, channels) group: one maximum call, then one gather per picture kind
  assert made == [(name, g) for g in (2, 2, 1, 1) for name in ('max', 'lut', 'lut')]
  for i, im in enumerate(images):  # argument order, whatever the grouping
    a = im[0].float().numpy()
    assert np.array_equal(lin[i].numpy(), encode(a)), i
    assert np.array_equal(tone[i].numpy(), encode(evaluate.tone_mapped_input(a))), i
    assert torch.equal(only[i], tone[i]) and torch.equal(again[0][i], lin[i]) and torch.equal(again[1][i], tone[i])


def _run(argv):
  with stand_ins(), mock.patch.object(evaluate, 'CLI_DEVICE', 'cpu'):
    return evaluate.main(argv)


@pytest.mark.parametrize('mode', [['--png'], ['--tiff16'], ['--device-png', '--step-by-step']])
@pytest.mark.parametrize('fused', [False, True])
def test_cli_device_input_png_writes_the_host_bytes(tmp_path, mode, fused):
  paths = fd._write_files(tmp_path)
  common = ['--seed', '3', '--dtype', 'f32', '--batch', '4', '--show-input', '--show-linear', *mode]
  host = _run(common + ['--device-decode', '--device-proxy', '--out', str(tmp_path / 'host') + os.sep] + paths)
  extra = ['--fused-decode'] if fused else ['--device-proxy']  # --device-input-png implies --device-decode
  del calls[:]
  dev = _run(common + extra + ['--device-input-png', '--out', str(tmp_path / 'dev') + os.sep] + paths)
  assert [name for name, _n in calls].count('lut') == 2 * [name for name, _n in calls].count('max') > 0
  assert len(host) == len(dev) == len(paths)
  for a, b in zip(host, dev):
    assert sorted(a['png']) == sorted(b['png']) and {'linear', 'input_tone_mapped'} <= set(b['png'])
    assert b['png']['linear'].endswith('.linear.png')
    for k in a['png']:
      assert open(a['png'][k], 'rb').read() == open(b['png'][k], 'rb').read(), k
  assert sorted(os.listdir(str(tmp_path / 'host'))) == sorted(os.listdir(str(tmp_path / 'dev')))


def test_cli_show_linear_on_the_host_path(tmp_path):
  """--show-linear without --device-input-png: save_png of the input, next to --show-input's picture; one flag alone
  writes one picture"""
  from PIL import Image
  paths = fd._write_files(tmp_path)[:2]
  rec = _run(['--seed', '3', '--png', '--show-linear', '--out', str(tmp_path / 'o') + os.sep] + paths)
  for r, p in zip(rec, paths):
    assert sorted(r['png']) == ['linear', 'retouched']
    want = encode(evaluate.load_image(p).astype(np.float16).astype(np.float32))  # (--dtype f16 storage)
    assert np.array_equal(np.asarray(Image.open(r['png']['linear'])), want)
  del calls[:]
  rec = _run(['--seed', '3', '--png', '--show-input', '--device-input-png', '--out', str(tmp_path / 'p') + os.sep] + paths)
  assert all(sorted(r['png']) == ['input_tone_mapped', 'retouched'] for r in rec)
  assert [name for name, _n in calls] == ['max', 'lut'] * len(paths)  # --batch 1: one group per image, one picture kind


@pytest.mark.parametrize('flags', [['--fused-decode', '--show-input'], ['--fused-decode', '--show-linear'],
                                   ['--fused-decode', '--masking'], ['--fused-decode', '--stepwise'],
                                   ['--fused-decode', '--stepwise', '--device-input-png', '--show-input'],
                                   ['--fused-decode', '--masking', '--device-input-png', '--show-linear']])
def test_cli_refusals_keep_their_message(tmp_path, flags, capsys):
  paths = fd._write_files(tmp_path)[:1]
  with pytest.raises(SystemExit):
    _run(flags + paths)
  assert '--fused-decode does not go with --stepwise, --masking or --show-input' in capsys.readouterr().err


@pytest.mark.parametrize('fused', [False, True])
def test_cli_uploads_the_codes_once(tmp_path, fused):
  """--device-input-png next to the decode or the pass from codes: one upload per image serves both"""
  paths = fd._write_files(tmp_path)
  real, seen = evaluate.upload_codes, []

  def counting(codes, device):
    seen.append(codes.shape)
    return real(codes, device)

  extra = ['--fused-decode'] if fused else ['--device-proxy']
  with mock.patch.object(evaluate, 'upload_codes', counting):
    _run(['--seed', '3', '--png', '--batch', '4', '--show-input', '--show-linear', '--device-input-png', *extra,
          '--out', str(tmp_path / 'o') + os.sep] + paths)
  assert len(seen) == len(paths)
