"""High-resolution inference loop (``/root/reference/net.py:711-821``, ``evaluate.py:8-31``).

Per image: a 64x64 proxy is made from the full-resolution picture (``net.py:779``: bilinear resize
of the centre crop), and for ``cfg.test_steps`` (= 5) steps the agent regresses parameters and picks
a filter on the PROXY while the same per-image parameters are applied to BOTH the proxy and the
full-resolution tensor (``filters.py:88-96``; ``agent.py:124-129``), feeding both outputs back
(``net.py:796-821``).  ``is_train = 0`` -> the action is ``argmax(pdf)`` (``agent.py:114-116``);
dropout stays on, as in the reference (``agent.py:36``), unless masks are passed.

Image decoding (16-bit TIFF / ProPhoto linearisation, ``util.py:311-323, 495-501``) sits in ``load_image``; of the
outputs of ``net.py:825-877`` the CLI writes the linear result (.npy) and, with ``--png``, the reference's 8-bit
``retouched`` / ``input_tone_mapped`` pictures; with ``--step-by-step`` also the ``intermediateNN`` pictures of
``net.py:820-823`` (``evaluate.py:31``); the debug pickle and the cv2-drawn ``steps`` panel are out of scope.
``--tiff16`` writes the pictures as 16-bit TIFFs instead, the depth the input files have; ``--device-jpeg-encode``
writes them as baseline JPEG files encoded on the GPU (``encode_jpeg_batch``); ``--device-jpeg-decode`` decodes
baseline JPEG inputs on the GPU from the files' bytes (``load_raws``, ``jpeg_decode.py``).
"""
import sys
import warnings

import numpy as np
import torch

from .util import STATE_STOPPED_DIM


def linearize_ProPhotoRGB(pp_rgb):
  """util.py:495-501 as used by net.py:733 (``reverse=False``): gamma 1.8 decode."""
  return pp_rgb**1.8


def get_image_center(image):
  """util.py:160-167: the largest centred square (NHWC)."""
  h, w = image.shape[1], image.shape[2]
  if h > w:
    o = (h - w) // 2
    return image[:, o:o + w]
  o = (w - h) // 2
  return image[:, :, o:o + h]


def make_low_res(high_res, size):
  """net.py:779: cv2.resize(get_image_center(hi), (size, size)) -- bilinear, half-pixel centres."""
  c = get_image_center(high_res).permute(0, 3, 1, 2).float()
  low = torch.nn.functional.interpolate(c, size=(size, size), mode='bilinear', align_corners=False,
                                        antialias=False)
  return low.permute(0, 2, 3, 1).contiguous().to(high_res.dtype)


def center_windows(shapes):
  """``get_image_center``'s slices as window rows: for every (H, W) of ``shapes`` the row (i, y0, x0, side) of the
  largest centred square of image i (what ``_cabi.bilinear_resize_ragged`` / ``area_resize_ragged`` take)."""
  rows = []
  for i, (h, w) in enumerate(shapes):
    h, w = int(h), int(w)
    rows.append((i, (h - w) // 2, 0, w) if h > w else (i, 0, (w - h) // 2, h))
  return rows


def make_low_res_batch(images, size):
  """``make_low_res`` of N images of ANY sizes in ONE call (``expo_bilinear_resize_ragged``): images are device tensors
  (H_i, W_i, 3) or (1, H_i, W_i, 3) of one dtype; returns the stacked (N, size, size, 3) proxies in that dtype.  The
  kernel reads the 4 size^2 taps of each image where they are: no fp32 copy of the centre square, no per-image launch.
  Its float32 operations are rounded one by one; torch's may be contracted, so a value can differ from
  ``make_low_res``'s in the last place."""
  from . import _cabi
  xs = [im.contiguous() for im in images]
  if not xs:
    raise ValueError('make_low_res_batch: no images')
  out = torch.empty((len(xs), size, size, 3), dtype=xs[0].dtype, device=xs[0].device)
  return _cabi.bilinear_resize_ragged(xs, center_windows([x.shape[-3:-1] for x in xs]), size, out)


PROXIES = ('torch', 'device')


def fused_chain(high_res, filter_ids, params24):
  """Apply a per-image sequence of filters to the full-resolution image in ONE pass
  (``expo_chain_fused_fwd``).  filter_ids: (N, steps) int32 C-ABI ids; params24: (N, steps, 24)."""
  from . import _cabi
  out = torch.empty_like(high_res)
  _cabi.chain_fused_fwd(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(),
                        high_res.contiguous(), out)
  return out


def fused_chain_ragged(images, filter_ids, params24):
  """``fused_chain`` over a list of images of different sizes in ONE ragged launch (``expo_chain_fused_fwd_ragged``):
  images: N device tensors (H_i, W_i, 3) or (1, H_i, W_i, 3), one dtype; row i of filter_ids (N, steps) / params24
  (N, steps, 24) is image i's sequence.  Returns the N outputs, each shaped like its input."""
  from . import _cabi
  xs = [im.contiguous() for im in images]
  ys = [torch.empty_like(x) for x in xs]
  _cabi.chain_fused_fwd_ragged(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(), xs, ys)
  return ys


def fused_chain_taps(high_res, filter_ids, params24, tap_mask, tap_dtype, out=True):
  """``fused_chain`` that also returns the image after every step k whose bit is set in ``tap_mask``, from the same
  pass (``expo_chain_fused_fwd_taps``): (out or None, taps (T, N, H, W, 3) of ``tap_dtype``: torch.uint8 for the 8-bit
  PNG values, torch.uint16 for the 16-bit TIFF values, else high_res's dtype)."""
  from . import _cabi
  x = high_res.contiguous()
  y = torch.empty_like(x) if out else None
  t = bin(tap_mask).count('1')
  taps = torch.empty((t,) + tuple(x.shape), dtype=tap_dtype, device=x.device)
  _cabi.chain_fused_fwd_taps(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(), x, y, tap_mask,
                             taps if t else None)
  return y, taps


def fused_chain_ragged_taps(images, filter_ids, params24, tap_mask, tap_dtype, out=True):
  """``fused_chain_ragged`` with taps (``expo_chain_fused_fwd_ragged_taps``): (outs or None, per image a (T, H_i, W_i,
  3) tensor of ``tap_dtype``), one ragged launch per 64 images."""
  from . import _cabi
  xs = [im.contiguous() for im in images]
  ys = [torch.empty_like(x) for x in xs] if out else None
  t = bin(tap_mask).count('1')
  taps = [torch.empty((t,) + tuple(x.shape[-3:]), dtype=tap_dtype, device=x.device) for x in xs]
  _cabi.chain_fused_fwd_ragged_taps(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(), xs, ys,
                                    tap_mask, taps if t else None)
  return ys, taps


def fused_masked_chain(high_res, filter_ids, params24, mask6, cfg, tap_mask=0, tap_dtype=None, out=True):
  """``fused_chain_taps`` with the spatial masks of ``cfg.masking`` (``expo_chain_fused_masked_fwd_ragged``): mask6
  (N, steps, 6) are the squashed mask rows the agent recorded (``debug_info['mask6']``).  The dense tensor goes in as N
  views of one ragged call; the taps come back as a (T, N, H, W, 3) view of an image-major buffer."""
  from . import _cabi
  x = high_res.contiguous()
  n, t = x.shape[0], bin(tap_mask).count('1')
  y = torch.empty_like(x) if out else None
  taps = torch.empty((n, t) + tuple(x.shape[1:]), dtype=tap_dtype or x.dtype, device=x.device)
  _cabi.chain_fused_masked_fwd_ragged(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(),
                                      mask6.contiguous().float(), list(x.unbind(0)),
                                      list(y.unbind(0)) if out else None, float(cfg.maximum_sharpness),
                                      float(cfg.minimum_strength), tap_mask, list(taps.unbind(0)) if t else None)
  return y, taps.transpose(0, 1)


def fused_masked_chain_ragged(images, filter_ids, params24, mask6, cfg, tap_mask=0, tap_dtype=None, out=True):
  """``fused_chain_ragged_taps`` with the spatial masks of ``cfg.masking``: (outs or None, per image a (T, H_i, W_i, 3)
  tensor of ``tap_dtype``), one ragged launch per 64 images."""
  from . import _cabi
  xs = [im.contiguous() for im in images]
  ys = [torch.empty_like(x) for x in xs] if out else None
  t = bin(tap_mask).count('1')
  taps = [torch.empty((t,) + tuple(x.shape[-3:]), dtype=tap_dtype or x.dtype, device=x.device) for x in xs]
  _cabi.chain_fused_masked_fwd_ragged(filter_ids.contiguous().to(torch.int32), params24.contiguous().float(),
                                      mask6.contiguous().float(), xs, ys, float(cfg.maximum_sharpness),
                                      float(cfg.minimum_strength), tap_mask, taps if t else None)
  return ys, taps


def fused_curves_chain(high_res, filter_ids, params48, curve_steps, tap_mask=0, tap_dtype=None, out=True):
  """``fused_chain_taps`` for any ``cfg.curve_steps`` (``expo_chain_fused_curves_fwd_ragged``): params48 (N, steps, 48)
  are the wide rows the agent recorded (``debug_info['params48']``), ``curve_steps`` the L the curve rows are packed
  for.  The dense tensor goes in as N views of one ragged call; the taps come back as a (T, N, H, W, 3) view of an
  image-major buffer."""
  from . import _cabi
  x = high_res.contiguous()
  n, t = x.shape[0], bin(tap_mask).count('1')
  y = torch.empty_like(x) if out else None
  taps = torch.empty((n, t) + tuple(x.shape[1:]), dtype=tap_dtype or x.dtype, device=x.device)
  _cabi.chain_fused_curves_fwd_ragged(filter_ids.contiguous().to(torch.int32), params48.contiguous().float(),
                                      int(curve_steps), list(x.unbind(0)), list(y.unbind(0)) if out else None, tap_mask,
                                      list(taps.unbind(0)) if t else None)
  return y, taps.transpose(0, 1)


def fused_curves_chain_ragged(images, filter_ids, params48, curve_steps, tap_mask=0, tap_dtype=None, out=True):
  """``fused_chain_ragged_taps`` for any ``cfg.curve_steps``: (outs or None, per image a (T, H_i, W_i, 3) tensor of
  ``tap_dtype``), one ragged launch per 64 images."""
  from . import _cabi
  xs = [im.contiguous() for im in images]
  ys = [torch.empty_like(x) for x in xs] if out else None
  t = bin(tap_mask).count('1')
  taps = [torch.empty((t,) + tuple(x.shape[-3:]), dtype=tap_dtype or x.dtype, device=x.device) for x in xs]
  _cabi.chain_fused_curves_fwd_ragged(filter_ids.contiguous().to(torch.int32), params48.contiguous().float(),
                                      int(curve_steps), xs, ys, tap_mask, taps if t else None)
  return ys, taps


def encode_u8(img):
  """``save_png``'s 8-bit encoding on the device: saturate(round_half_even(float(img) * 255))."""
  return torch.round(img.float() * 255.0).clamp_(0, 255).to(torch.uint8)


def encode_u16(img):
  """The 16-bit encoding of ``--tiff16`` on the device: saturate(round_half_even(float(img) * 65535)), what an
  EXPO_TAP_U16 tap holds.  The codes leave as the low halves of int32 values: a float -> uint16 cast is not relied on."""
  codes = torch.round(img.float() * 65535.0).clamp_(0, 65535).to(torch.int32).contiguous()
  return codes.view(torch.int16)[..., ::2].contiguous().view(torch.uint16)  # (little-endian host and device)


INTERMEDIATES = (None, 'u8', 'u16', 'storage')
PICTURES = (False, True, 'u8', 'u16')
MASKS = ('stepwise', 'fused')
CURVES = ('stepwise', 'fused')
_CODE_DTYPES = {'u8': torch.uint8, 'u16': torch.uint16}
_ENCODERS = {'u8': encode_u8, 'u16': encode_u16}


def _picture_kind(picture, intermediates):
  """``picture=`` as None / 'u8' / 'u16' (True is 'u8').  The taps of a launch share one format, and so do the pictures
  of a call: 'u8' and 'u16' do not mix."""
  if isinstance(picture, str):
    if picture not in _CODE_DTYPES:
      raise ValueError('picture must be one of %s' % (PICTURES,))
    kind = picture
  else:
    kind = 'u8' if picture else None
  if kind and intermediates in _CODE_DTYPES and intermediates != kind:
    raise ValueError('picture=%r and intermediates=%r: one call makes pictures of one depth' % (picture, intermediates))
  return kind


def _intermediate_mask(stops):
  """bit i: step i ran and the image was not stopped after it -- the steps net.py:820-823 saves a picture of"""
  return sum(1 << i for i, stopped in enumerate(stops) if not stopped)


def _agent_steps(agent, low, z, steps, dropout_masks, hi=None, generic=False, keep_hi=False, mask6=None, params48=None):
  """The agent loop of ``retouch`` on the (N, 64, 64, 3) proxies: ``steps`` steps (or until every image stopped), the
  full-resolution tensor ``hi`` filtered at every step when given (the reference's schedule).  Returns low, states,
  hi, and per step the selected ids, the C-ABI ids, the (N, 24) parameter rows, whether every image was stopped after
  it and (``keep_hi``) the full-resolution tensor after it.  ``mask6``: a list that receives every step's (N, 6)
  squashed mask rows when the agent reports them (``cfg.masking``).  ``params48``: a list that receives every step's
  (N, 48) wide parameter rows of a ``generic`` agent, whose C-ABI ids are then the ones it reports."""
  cfg = agent.cfg
  n, dev = low.shape[0], low.device
  states = torch.zeros((n, cfg.num_state_dim), dtype=torch.float32, device=dev)  # get_initial_states
  trace, abi_ids, params, stops, his = [], [], [], [], []
  for i in range(steps):
    masks = dropout_masks[i] if dropout_masks is not None else None
    if hi is None:
      (low, states, _s, _p), dbg, _ = agent((low, z, states), is_train=0, progress=0.0, dropout_masks=masks)
    else:
      (low, states, hi), dbg, _ = agent((low, z, states), is_train=0, progress=0.0, high_res=hi,
                                        dropout_masks=masks)
    if generic:  # no (N, 24) parameter rows exist for this configuration: record the ids only
      if params48 is not None:  # (and the rows of the fused pass for any curve_steps)
        abi_ids.append(dbg['abi_filter_ids'])
        params48.append(dbg['params48'])
      else:
        abi_ids.append(agent.abi_filter_ids[dbg['selected_filter_ids'].clamp_min(0).long()])
      params.append(torch.zeros((n, 24), dtype=torch.float32, device=dev))
    else:
      abi_ids.append(dbg['abi_filter_ids'])
      params.append(dbg['params24'])
    trace.append(dbg['selected_filter_ids'].clone())
    if mask6 is not None and 'mask6' in dbg:
      mask6.append(dbg['mask6'])
    if keep_hi:
      his.append(hi)
    stops.append(bool((states[:, STATE_STOPPED_DIM] > 0).all()))
    if stops[-1]:
      break
  return low, states, hi, trace, abi_ids, params, stops, his


def _trace_result(out, low, states, trace, abi_ids, params, return_trace, mask6=(), params48=()):
  if return_trace == 'full':  # the per-step operations (what net.py:825-877 pickles as decisions / operations)
    ops = dict(selected=torch.stack(trace, dim=1), abi_filter_ids=torch.stack(abi_ids, dim=1),
               params24=torch.stack(params, dim=1))
    if mask6:  # cfg.masking: the (N, S, 6) squashed mask rows of the selected filters
      ops['mask6'] = torch.stack(mask6, dim=1)
    if params48:  # curves='fused': the (N, S, 48) rows fused_curves_chain replays (params24 is all zero then)
      ops['params48'] = torch.stack(params48, dim=1)
    return out, low, states, ops
  if return_trace:
    return out, low, states, torch.stack(trace, dim=1)
  return out, low, states


@torch.no_grad()
def retouch(agent, high_res, steps=None, z=None, dropout_masks=None, return_trace=False, fused=True,
            intermediates=None, proxy='torch', picture=False, masks='stepwise', curves='stepwise'):
  """Run the 5-step retouching loop.  ``high_res``: NHWC device tensor (fp16/fp32), linear RGB.
  Returns (retouched_high_res, retouched_low_res, states[, trace of selected filter ids][, intermediates]).

  ``intermediates='u8'`` / ``'u16'`` / ``'storage'`` adds the step-by-step pictures of ``net.py:820-823``: a
  (S-1, N, H, W, 3) tensor (with the shipped agent every step but the last; in general every step after which the
  images were not stopped), uint8 ``save_png`` values, uint16 ``encode_u16`` values or the storage dtype.  On the fused path they come from the same pass
  (``fused_chain_taps``); otherwise they are the per-step tensors, encoded on the device.

  ``fused=True`` (default): the agent steps run on the 64x64 proxy only, recording each step's
  (filter id, parameters); the full-resolution image is then read once, pushed through all steps
  in registers and written once.  ``fused=False`` is the reference's schedule (``net.py:796-821``):
  every step also filters the full-resolution tensor and feeds it back -- identical maths, one
  fp16 rounding per step, ``steps`` times the HBM traffic.

  ``proxy='device'`` makes the 64x64 proxies with ``make_low_res_batch`` (one HIP launch) instead of torch's
  interpolate; ``'torch'`` (default) is ``make_low_res``.  ``picture=True`` appends the (N, H, W, 3) uint8 picture of
  the result (``save_png``'s encoding) as the last entry: on the fused path an EXPO_TAP_U8 tap of the last executed
  step, written by the pass that writes the output; otherwise ``encode_u8`` of it.  ``picture='u8'`` is the same;
  ``picture='u16'`` makes it the uint16 picture (EXPO_TAP_U16 / ``encode_u16``: with fp16 storage it carries fp16's 11
  significant bits, the full 16-bit depth needs fp32 storage).  'u8' and 'u16' do not mix in one call (``ValueError``).

  ``masks`` matters with ``cfg.masking`` only.  ``'stepwise'`` (default): the reference's schedule, as ``fused=False``.
  ``'fused'``: the spatial mask of a step needs the pixel's position, the running value's luminance and six numbers the
  agent regresses on the proxy, so the fused pass takes it too (``fused_masked_chain``): the agent runs on the proxies
  only, and intermediates, picture and trace come as on the unmasked fused path.  fp32 between steps instead of one
  storage rounding per step.  ``fused=False`` wins over it.

  ``curves`` matters only for an agent with a generic curve filter (``cfg.curve_steps != 8``).  ``'stepwise'`` (default):
  the reference's schedule on the generic kernels, as ``fused=False``.  ``'fused'``: the agent runs on the proxies only,
  recording each step's C-ABI id and wide parameter row (``debug_info['params48']``), and ``fused_curves_chain`` applies
  them in one pass; intermediates, picture and trace come as on the 8-step fused path, and a ``'full'`` trace also
  carries ``params48`` (N, S, 48).  ``fused=False`` wins over it, and ``cfg.masking`` keeps the stepwise schedule."""
  cfg = agent.cfg
  if intermediates not in INTERMEDIATES:
    raise ValueError('intermediates must be one of %s' % (INTERMEDIATES,))
  if proxy not in PROXIES:
    raise ValueError('proxy must be one of %s' % (PROXIES,))
  if masks not in MASKS:
    raise ValueError('masks must be one of %s' % (MASKS,))
  if curves not in CURVES:
    raise ValueError('curves must be one of %s' % (CURVES,))
  kind = _picture_kind(picture, intermediates)
  if cfg.masking and masks != 'fused':
    fused = False  # the reference's schedule: every step filters the full-resolution tensor
  generic = any(f.uses_generic_kernels() for f in agent.filters)
  fused_curves = generic and fused and curves == 'fused' and not cfg.masking
  if generic and not fused_curves:
    fused = False  # cfg.curve_steps != 8: the one-pass kernel is instantiated for 8-step curves (reference schedule instead)
  steps = steps or cfg.test_steps
  n = high_res.shape[0]
  dev = high_res.device
  if proxy == 'device':
    low = make_low_res_batch(list(high_res.unbind(0)), cfg.source_img_size)
  else:
    low = make_low_res(high_res, cfg.source_img_size)
  if z is None:
    z = torch.rand((n, cfg.z_dim), device=dev)
  hi = high_res.contiguous()
  mask6, wide = [], []
  low, states, stepped, trace, abi_ids, params, stops, his = _agent_steps(
      agent, low, z, steps, dropout_masks, hi=None if fused else hi, generic=generic,
      keep_hi=bool(intermediates) and not fused, mask6=mask6, params48=wide if fused_curves else None)
  rows = wide if fused_curves else params  # the parameter rows of the fused pass
  mask = _intermediate_mask(stops)
  inter = pic = None
  last = 1 << (len(stops) - 1)  # the last executed step: its u8 / u16 tap is the picture of the output
  if fused and cfg.masking:  # the same pass with the spatial masks
    def chain_taps(x, ids, prm, tap_mask, tap_dtype):
      return fused_masked_chain(x, ids, prm, torch.stack(mask6, dim=1), cfg, tap_mask, tap_dtype)
  elif fused_curves:  # the same pass for this cfg.curve_steps
    def chain_taps(x, ids, prm, tap_mask, tap_dtype):
      return fused_curves_chain(x, ids, prm, cfg.curve_steps, tap_mask, tap_dtype)
  else:
    chain_taps = fused_chain_taps
  if fused and kind and intermediates != 'storage':
    # one pass: the output, the picture and (u8 / u16) the intermediates, which are the taps before the last
    hi, taps = chain_taps(hi, torch.stack(abi_ids, dim=1), torch.stack(rows, dim=1),
                          (mask if intermediates else 0) | last, _CODE_DTYPES[kind])
    pic = taps[-1]
    if intermediates:
      inter = taps if mask & last else taps[:-1]
  elif fused and intermediates:
    hi, inter = chain_taps(hi, torch.stack(abi_ids, dim=1), torch.stack(rows, dim=1), mask,
                           _CODE_DTYPES.get(intermediates, hi.dtype))
  elif fused and (cfg.masking or fused_curves):
    hi, _ = chain_taps(hi, torch.stack(abi_ids, dim=1), torch.stack(rows, dim=1), 0, None)
  elif fused:
    hi = fused_chain(hi, torch.stack(abi_ids, dim=1), torch.stack(params, dim=1))
  else:
    hi = stepped
    if intermediates:
      kept = [h for i, h in enumerate(his) if (mask >> i) & 1]
      inter = torch.stack(kept) if kept else torch.empty((0,) + tuple(hi.shape), dtype=hi.dtype, device=hi.device)
      if intermediates in _ENCODERS:
        inter = _ENCODERS[intermediates](inter)
  if kind and pic is None:
    pic = _ENCODERS[kind](hi)
  res = _trace_result(hi, low, states, trace, abi_ids, params, return_trace, mask6, wide)
  return res + ((inter,) if intermediates else ()) + ((pic,) if kind else ())


@torch.no_grad()
def retouch_batch(agent, images, steps=None, z=None, dropout_masks=None, return_trace=False, intermediates=None,
                  proxy='torch', picture=False, masks='stepwise', curves='stepwise'):
  """``retouch`` over a list of images of ANY sizes at once (the batching ``evaluate.py:18`` asks for, without its
  same-resolution restriction).  ``images``: N device tensors (H_i, W_i, 3) or (1, H_i, W_i, 3), one dtype and device.
  One 64x64 proxy per image (``make_low_res``) is stacked, the agent runs once on the (N, 64, 64, 3) stack, and the
  recorded sequences are applied to the full-resolution images in ONE ragged launch (``fused_chain_ragged``).  ``z``
  (N, z_dim) and ``dropout_masks`` (per step, (N, ...) rows) as in ``retouch``.  Stopping is uniform across a batch
  (``submitted = is_last_step``), so every image runs the same number of steps.

  Returns (list of N outputs shaped like their inputs, low (N, 64, 64, 3), states (N, D)[, trace]) with the trace in
  ``retouch``'s shapes.  Where ``retouch`` cannot fuse (``cfg.masking``, or ``cfg.curve_steps != 8``: the reference's
  schedule on the generic kernels) every image goes through ``retouch`` alone, with its rows of ``z`` and masks (z is
  still drawn once for the batch when not given), and the per-image results are concatenated.

  ``intermediates`` as in ``retouch`` appends a list of N (S-1, H_i, W_i, 3) tensors; on the fused path they come from
  the ragged launch itself (``fused_chain_ragged_taps``).  ``proxy`` and ``picture`` as in ``retouch``: ``'device'``
  builds all N proxies in one launch (``make_low_res_batch``) instead of ``make_low_res`` per image, and
  ``picture=True`` appends a list of N (H_i, W_i, 3) uint8 pictures, from the ragged launch that writes the outputs
  (``'u16'``: uint16 pictures).

  ``masks='fused'`` with ``cfg.masking`` keeps the batch together as without masks: one agent call on the stacked
  proxies, then ``fused_masked_chain_ragged`` (see ``retouch``); the default ``'stepwise'`` runs every image alone.
  ``curves='fused'`` does the same for an agent with generic curve filters (``cfg.curve_steps != 8``, masking off):
  one agent call, then ``fused_curves_chain_ragged``; the default ``'stepwise'`` runs every image alone."""
  cfg = agent.cfg
  if intermediates not in INTERMEDIATES:
    raise ValueError('intermediates must be one of %s' % (INTERMEDIATES,))
  if proxy not in PROXIES:
    raise ValueError('proxy must be one of %s' % (PROXIES,))
  if masks not in MASKS:
    raise ValueError('masks must be one of %s' % (MASKS,))
  if curves not in CURVES:
    raise ValueError('curves must be one of %s' % (CURVES,))
  kind = _picture_kind(picture, intermediates)
  images = list(images)
  n = len(images)
  if n == 0:
    raise ValueError('retouch_batch: no images')
  dev = images[0].device
  for im in images:
    if im.dtype != images[0].dtype or im.device != dev or im.shape[-1] != 3 or not (
        im.dim() == 3 or (im.dim() == 4 and im.shape[0] == 1)):
      raise ValueError('retouch_batch: images must be (H, W, 3) or (1, H, W, 3) tensors of one dtype and device')
  steps = steps or cfg.test_steps
  if z is None:
    z = torch.rand((n, cfg.z_dim), device=dev)
  hi4 = [im if im.dim() == 4 else im[None] for im in images]
  generic = any(f.uses_generic_kernels() for f in agent.filters)
  fused_curves = generic and curves == 'fused' and not cfg.masking
  if (cfg.masking and masks != 'fused') or (generic and not fused_curves):  # per image, the schedule retouch picks for it
    rows = []
    for i, im in enumerate(hi4):
      drop = None if dropout_masks is None else [tuple(m[i:i + 1] for m in step) for step in dropout_masks]
      rows.append(retouch(agent, im, steps=steps, z=z[i:i + 1], dropout_masks=drop, return_trace=return_trace or True,
                          intermediates=intermediates, proxy=proxy, picture=picture, masks=masks, curves=curves))
    outs = [r[0].reshape(im.shape) for r, im in zip(rows, images)]
    low, states = torch.cat([r[1] for r in rows]), torch.cat([r[2] for r in rows])
    extra = ([r[4][:, 0] for r in rows],) if intermediates else ()
    if kind:
      extra += ([r[-1][0] for r in rows],)
    if return_trace == 'full':
      return (outs, low, states, {k: torch.cat([r[3][k] for r in rows]) for k in rows[0][3]}) + extra
    if return_trace:
      return (outs, low, states, torch.cat([r[3] for r in rows])) + extra
    return (outs, low, states) + extra
  if proxy == 'device':
    low = make_low_res_batch(images, cfg.source_img_size)
  else:
    low = torch.cat([make_low_res(im, cfg.source_img_size) for im in hi4])
  mask6, wide = [], []
  low, states, _hi, trace, abi_ids, params, stops, _his = _agent_steps(
      agent, low, z, steps, dropout_masks, generic=generic, mask6=mask6, params48=wide if fused_curves else None)
  ids, prm = torch.stack(abi_ids, dim=1), torch.stack(wide if fused_curves else params, dim=1)
  if cfg.masking:  # the same launches with the spatial masks
    def ragged_taps(xs, ids, prm, tap_mask, tap_dtype):
      return fused_masked_chain_ragged(xs, ids, prm, torch.stack(mask6, dim=1), cfg, tap_mask, tap_dtype)
  elif fused_curves:  # the same launches for this cfg.curve_steps
    def ragged_taps(xs, ids, prm, tap_mask, tap_dtype):
      return fused_curves_chain_ragged(xs, ids, prm, cfg.curve_steps, tap_mask, tap_dtype)
  else:
    ragged_taps = fused_chain_ragged_taps
  if kind and intermediates != 'storage':
    # one ragged launch: the outputs, the pictures and (u8 / u16) the intermediates, which are the taps before the last
    mask, last = _intermediate_mask(stops), 1 << (len(stops) - 1)
    outs, taps = ragged_taps(images, ids, prm, (mask if intermediates else 0) | last, _CODE_DTYPES[kind])
    res = _trace_result(outs, low, states, trace, abi_ids, params, return_trace, mask6, wide)
    if intermediates:
      res += ([t if mask & last else t[:-1] for t in taps],)
    return res + ([t[-1] for t in taps],)
  if kind:  # storage intermediates: the taps of a launch have one format, so the pictures are encoded from the outputs
    outs, inter = ragged_taps(images, ids, prm, _intermediate_mask(stops), images[0].dtype)
    res = _trace_result(outs, low, states, trace, abi_ids, params, return_trace, mask6, wide)
    return res + (inter, [_ENCODERS[kind](o.reshape(o.shape[-3:])) for o in outs])
  if not intermediates:
    outs = ragged_taps(images, ids, prm, 0, None)[0] if cfg.masking or fused_curves else \
        fused_chain_ragged(images, ids, prm)
    return _trace_result(outs, low, states, trace, abi_ids, params, return_trace, mask6, wide)
  outs, inter = ragged_taps(images, ids, prm, _intermediate_mask(stops),
                            _CODE_DTYPES.get(intermediates, images[0].dtype))
  return _trace_result(outs, low, states, trace, abi_ids, params, return_trace, mask6, wide) + (inter,)


def load_image(path):
  """net.py:726-747: ``.tif`` -> 16-bit ProPhoto, linearised (x**1.8); anything else readable by
  PIL -> sRGB-ish: ``/255`` (uint8) or ``/65535`` (uint16), ``**2.2``, scaled by ``1 / (2 max)``."""
  import numpy as np
  if path.lower().endswith(('.tif', '.tiff')):
    from .tiff16 import read_tiff16
    return linearize_ProPhotoRGB(read_tiff16(path))
  from PIL import Image
  pil = Image.open(path)
  raw = np.asarray(pil)
  if raw.dtype == np.uint16:  # net.py:738-739 (16-bit grey / multi-channel arrays PIL can deliver)
    img = raw.astype(np.float32) / 65535.0
    if img.ndim == 2:
      img = np.repeat(img[:, :, None], 3, axis=2)
    img = img[:, :, :3]
  else:
    img = np.asarray(pil.convert('RGB'), dtype=np.float32) / 255.0
  img = img**2.2  # linearise sRGB
  return img / (2 * img.max())  # mimic RAW exposure


DECODE_KINDS = ('srgb8', 'srgb16', 'prophoto16')
DECODE_NORMALIZE = {'srgb8': 1, 'srgb16': 1, 'prophoto16': 0}  # load_image scales the sRGB kinds by 1 / (2 max)


def load_raw(path):
  """``load_image``'s file-level choices without its float maths: (codes (H, W, C) uint8 / uint16 as the file holds
  them, kind).  ``.tif`` -> the 16-bit samples, 'prophoto16'; a PIL uint16 array -> 'srgb16' (2-D: C = 1); anything
  else -> ``pil.convert('RGB')``, 'srgb8'.  ``decode_images`` turns them into what ``load_image`` returns."""
  if path.lower().endswith(('.tif', '.tiff')):
    from .tiff16 import read_tiff
    raw = read_tiff(path)
    if raw.dtype != np.uint16:
      raise ValueError('expected a 16-bit TIFF')
    return raw, 'prophoto16'
  from PIL import Image
  pil = Image.open(path)
  raw = np.asarray(pil)
  if raw.dtype == np.uint16:
    return (raw[:, :, None] if raw.ndim == 2 else raw), 'srgb16'
  return np.asarray(pil.convert('RGB')), 'srgb8'


def load_raws(paths, device=None, device_jpeg=False, jpeg_sync='auto'):
  """``load_raw`` of every path.  With ``device_jpeg`` every ``.jpg`` / ``.jpeg`` path that
  ``jpeg_decode.parse`` accepts is read as bytes and decoded on ``device`` in one batch call: its codes are an
  (H, W, 3) uint8 device tensor, bit for bit ``load_raw``'s array, kind 'srgb8', and never visit the host.  Every other
  path goes through ``load_raw``; one line on stderr names those files and why."""
  if not device_jpeg:
    return [load_raw(path) for path in paths]
  from . import jpeg_decode
  raws, datas, plans, where, fell = [None] * len(paths), [], [], [], []
  for i, path in enumerate(paths):
    if not jpeg_decode.is_jpeg_path(path):
      fell.append('%s (not a .jpg / .jpeg path)' % path)
      continue
    with open(path, 'rb') as f:
      data = f.read()
    try:
      plans.append(jpeg_decode.parse(data))
    except jpeg_decode.UnsupportedJpeg as e:
      fell.append('%s (%s)' % (path, e))
      continue
    datas.append(data)
    where.append(i)
  if fell:
    print('--device-jpeg-decode: decoded on the host: ' + ', '.join(fell), file=sys.stderr)
  codes, _ = jpeg_decode.decode_jpeg_batch(datas, device, plans=plans, names=[paths[i] for i in where], sync=jpeg_sync)
  for i, c in zip(where, codes):
    raws[i] = (c, 'srgb8')
  return [load_raw(path) if raw is None else raw for path, raw in zip(paths, raws)]


_DECODE_TABLES = {}


def decode_table(kind, device):
  """The float32 linearisation of every code of ``kind``: ``load_image``'s own expression evaluated on the code range
  (cached per kind and device)."""
  key = (kind, torch.device(device))
  t = _DECODE_TABLES.get(key)
  if t is None:
    if kind == 'srgb8':
      a = (np.arange(256, dtype=np.float32) / 255.0)**2.2
    elif kind == 'srgb16':
      a = (np.arange(65536, dtype=np.float32) / 65535.0)**2.2
    elif kind == 'prophoto16':
      a = linearize_ProPhotoRGB(np.arange(65536, dtype=np.float32) / 65535.0)
    else:
      raise ValueError('decode kind must be one of %s, got %r' % (DECODE_KINDS, kind))
    t = _DECODE_TABLES[key] = torch.from_numpy(a).to(key[1])
  return t


def upload_codes(codes, device):
  """The codes of one ``load_raw`` result on the device, as they are (PIL's arrays are read-only: they are only read).
  Codes that are on a device already (``load_raws`` with ``device_jpeg``) pass through."""
  if isinstance(codes, torch.Tensor):
    return codes
  with warnings.catch_warnings():
    warnings.simplefilter('ignore', UserWarning)
    return torch.from_numpy(np.ascontiguousarray(codes)).to(device)


def decode_images(raws, dtype, device, staged=None):
  """``load_image`` + ``.to(dtype)`` on the device from ``load_raw`` results: the codes are uploaded as they are and
  ``_cabi.decode_ragged`` makes the linear storage tensors, bit for bit what the host path gives.  One ragged call
  per distinct (kind, channels); returns (1, H, W, 3) tensors in the order of ``raws``.  ``staged``: the listed result
  of ``stage_raws`` for these ``raws``; its uploaded codes are decoded instead of a second upload."""
  from . import _cabi
  dev = torch.device(device)
  outs = [None] * len(raws)
  if staged is None:
    groups = {}
    for i, (codes, kind) in enumerate(raws):
      groups.setdefault((kind, codes.shape[2]), []).append(i)
    staged = ((idx, [upload_codes(raws[i][0], dev) for i in idx], None, None, kind) for (kind, _c), idx in groups.items())
  for idx, cs, _tables, _stride, kind in staged:
    ys = [torch.empty((1, c.shape[0], c.shape[1], 3), dtype=dtype, device=dev) for c in cs]
    _cabi.decode_ragged(cs, decode_table(kind, dev), DECODE_NORMALIZE[kind], ys)
    for i, y in zip(idx, ys):
      outs[i] = y
  return outs


def stage_raws(raws, dtype, device):
  """The upload-and-tables staging the passes from codes share: per (kind, channels) group of ``raws`` (``load_raw``
  results), in order of first appearance, yields (the images' indices, their codes on the device, the tables
  ``decode_ragged`` would gather from in ``dtype``, the tables' stride, the kind).  A generator: a consumer may work on
  a group before the next one is staged; ``list(stage_raws(...))`` can be handed to ``retouch_batch_raw`` and
  ``input_pictures_raw`` (``staged=``), so the codes are uploaded once for both."""
  from . import _cabi
  dev = torch.device(device)
  groups = {}
  for i, (codes, k) in enumerate(raws):
    groups.setdefault((k, codes.shape[2]), []).append(i)
  for (k, _c), idx in groups.items():
    cs = [upload_codes(raws[i][0], dev) for i in idx]
    tables, stride = _cabi.decode_tables(cs, decode_table(k, dev), DECODE_NORMALIZE[k], dtype)
    yield idx, cs, tables, stride, k


@torch.no_grad()
def retouch_batch_raw(agent, raws, dtype, device, steps=None, z=None, dropout_masks=None, return_trace=False,
                      intermediates=None, picture=False, outputs=True, staged=None, curves='stepwise'):
  """``retouch_batch(agent, decode_images(raws, dtype, device), proxy='device', ...)`` without the decoded tensors
  (DESIGN.md §3.23): ``raws`` are ``load_raw`` results, and the integer codes are what the device reads.  Per
  (kind, channels) group of the batch ``_cabi.decode_tables`` writes the tables ``decode_ragged`` would gather from
  (``stage_raws``; ``staged=`` takes its listed result instead); then the 64x64 proxies of the whole batch, stacked in
  argument order, come from one ``_cabi.bilinear_resize_ragged_codes`` call per group, the agent runs once, and one
  ``_cabi.chain_fused_fwd_ragged_codes`` launch per group applies that group's rows of ids and params to the codes.
  Every returned value is bit for bit the one of the call above.

  ``curves='fused'`` serves an agent with generic curve filters (a ``cfg.curve_steps`` other than 8)
  the same way: the agent records its 48-wide rows (``_agent_steps(..., generic=True, params48=...)``, as
  ``retouch_batch`` does for ``curves='fused'``) and one ``_cabi.chain_fused_curves_fwd_ragged_codes`` launch per group
  applies them.  Every returned value is then bit for bit the one of
  ``retouch_batch(agent, decode_images(raws, dtype, device), proxy='device', curves='fused', ...)``.  With an 8-step
  agent ``curves`` has no effect.

  ``outputs=False`` allocates no float output: the first entry is a list of ``None`` (it needs ``picture`` or
  ``intermediates``: something must be written).  ``cfg.masking``, or a ``cfg.curve_steps`` that needs the generic
  kernels under the default ``curves='stepwise'``, raises ``ValueError``: there is no pass from codes for them and no
  silent fallback."""
  from . import _cabi
  cfg = agent.cfg
  if intermediates not in INTERMEDIATES:
    raise ValueError('intermediates must be one of %s' % (INTERMEDIATES,))
  if curves not in CURVES:
    raise ValueError('curves must be one of %s' % (CURVES,))
  kind = _picture_kind(picture, intermediates)
  if cfg.masking:
    raise ValueError('retouch_batch_raw: cfg.masking has no pass from codes (decode_images + retouch_batch)')
  generic = any(f.uses_generic_kernels() for f in agent.filters)
  if generic and curves != 'fused':
    raise ValueError('retouch_batch_raw: cfg.curve_steps = %s needs the generic kernels, which have no step-by-step '
                     'pass from codes (curves=\'fused\', or decode_images + retouch_batch)' % (cfg.curve_steps,))
  raws = list(raws)
  n = len(raws)
  if n == 0:
    raise ValueError('retouch_batch_raw: no images')
  if not outputs and not kind and not intermediates:
    raise ValueError('retouch_batch_raw: outputs=False needs picture or intermediates (nothing would be written)')
  dev = torch.device(device)
  steps = steps or cfg.test_steps
  if z is None:
    z = torch.rand((n, cfg.z_dim), device=dev)
  size = cfg.source_img_size
  low = torch.empty((n, size, size, 3), dtype=dtype, device=dev)
  groups = []  # per group: the images' indices, their codes on the device, the tables and their stride
  for idx, cs, tables, stride, _k in (stage_raws(raws, dtype, dev) if staged is None else staged):
    part = low if len(idx) == n else torch.empty((len(idx), size, size, 3), dtype=dtype, device=dev)
    _cabi.bilinear_resize_ragged_codes(cs, tables, stride, center_windows([c.shape[:2] for c in cs]), size, part)
    if part is not low:
      low[torch.tensor(idx, device=dev)] = part
    groups.append((idx, cs, tables, stride))
  wide = []
  low, states, _hi, trace, abi_ids, params, stops, _his = _agent_steps(
      agent, low, z, steps, dropout_masks, generic=generic, params48=wide if generic else None)
  ids, prm = torch.stack(abi_ids, dim=1), torch.stack(wide if generic else params, dim=1)
  mask, last = _intermediate_mask(stops), 1 << (len(stops) - 1)
  # the taps of a launch have one format: with storage intermediates the pictures are encoded from the outputs
  encode = kind and intermediates == 'storage'
  if kind and not encode:
    tap_mask, tap_dtype = (mask if intermediates else 0) | last, _CODE_DTYPES[kind]
  elif intermediates:
    tap_mask, tap_dtype = mask, _CODE_DTYPES.get(intermediates, dtype)
  else:
    tap_mask, tap_dtype = 0, None
  if encode and not outputs:
    raise ValueError('retouch_batch_raw: a picture next to storage intermediates is encoded from the output '
                     '(outputs=False cannot make it)')
  t = bin(tap_mask).count('1')
  outs, taps = [None] * n, [None] * n
  for idx, cs, tables, stride in groups:
    ys = [torch.empty((1, c.shape[0], c.shape[1], 3), dtype=dtype, device=dev) for c in cs] if outputs else None
    tp = [torch.empty((t, c.shape[0], c.shape[1], 3), dtype=tap_dtype, device=dev) for c in cs] if t else None
    sel = torch.tensor(idx, device=dev)
    whole = len(idx) == n
    gi, gp = (ids, prm) if whole else (ids[sel].contiguous(), prm[sel].contiguous())
    if generic:  # the same launch for this cfg.curve_steps
      _cabi.chain_fused_curves_fwd_ragged_codes(gi, gp, cfg.curve_steps, cs, tables, stride, ys, tap_mask, tp)
    else:
      _cabi.chain_fused_fwd_ragged_codes(gi, gp, cs, tables, stride, ys, tap_mask, tp)
    for j, i in enumerate(idx):
      if outputs:
        outs[i] = ys[j]
      if t:
        taps[i] = tp[j]
  res = _trace_result(outs, low, states, trace, abi_ids, params, return_trace, params48=wide)
  if kind and not encode:
    if intermediates:
      res += ([tp if mask & last else tp[:-1] for tp in taps],)
    return res + ([tp[-1] for tp in taps],)
  if intermediates:
    res += (taps,)
  if encode:
    res += ([_ENCODERS[kind](o.reshape(o.shape[-3:])) for o in outs],)
  return res


INPUT_CODES = {'u8': (np.uint8, 255.0), 'u16': (np.uint16, 65535.0)}


def input_luts(tables, stride, maxima, code='u8'):
  """The integer tables of the reference's two input pictures (``GAN.eval``, ``net.py:825-839``) over the code range,
  per image: (linear, tone_mapped), two (N, 2^bits) NumPy arrays of uint8 (``code='u8'``) or uint16 (``'u16'``).
  ``tables`` / ``stride`` are what ``_cabi.decode_tables`` returned (the storage-dtype tables, image i's row at entry
  i * stride; stride 0: one shared row), ``maxima`` the N largest codes of ``_cabi.codes_max_ragged``.  With
  t = float32(table of image i) -- the values the decoded image holds, code by code -- the tables are the project's own
  host expressions evaluated on t:
    linear       ``save_png``'s encoding of t                                     clip(rint(t * 255))
    tone_mapped  ``save_png``'s encoding of ``tone_mapped_input``'s expression    clip(rint((t / t[m_i]) ** (1 / 2.4) * 255))
  with ``a.max()`` = t[m_i]: the tables are non-decreasing, so the decoded image's largest value sits at its largest
  code.  ``'u16'`` uses ``encode_u16``'s scale 65535 instead of 255.  A picture is then a gather by code
  (``_cabi.codes_lut_ragged``), bit for bit ``save_png``'s encoding of the decoded image's pictures.

  An image whose divisor t[m_i] is 0 or NaN -- all-zero codes: the reference divides by zero there, and a normalised
  table is NaN throughout -- gets tables of 0 for both pictures."""
  ct, scale = INPUT_CODES[code]
  t = tables.detach().float().cpu().numpy()
  t = t.reshape(-1, t.shape[-1])
  m = np.asarray(maxima.cpu() if isinstance(maxima, torch.Tensor) else maxima).astype(np.int64).reshape(-1)
  entries = t.shape[-1]
  lin = np.zeros((len(m), entries), dtype=ct)
  tone = np.zeros((len(m), entries), dtype=ct)
  top = float(np.iinfo(ct).max)
  for i, mi in enumerate(m):
    a = t[(i * int(stride)) // entries]
    d = a[mi]
    if d == 0 or np.isnan(d):
      continue
    lin[i] = np.clip(np.rint(a * scale), 0, top).astype(ct)
    tone[i] = np.clip(np.rint(((a / d)**(1 / 2.4)) * scale), 0, top).astype(ct)
  return lin, tone


@torch.no_grad()
def input_pictures_raw(raws, dtype, device, linear=True, tone_mapped=True, code='u8', staged=None):
  """The reference's ``linear`` and ``input_tone_mapped`` pictures of ``load_raw`` results, made on the device from the
  integer codes: per (kind, channels) group one ``_cabi.codes_max_ragged``, the group's tables from
  ``input_luts`` uploaded, and one ``_cabi.codes_lut_ragged`` per requested picture kind.  Returns one list per requested
  kind, in the order (linear, tone_mapped): N device tensors (H_i, W_i, 3) of uint8 (``code='u8'``) or uint16, in the
  order of ``raws``; each equals ``save_png``'s encoding (``'u16'``: ``encode_u16``'s) of the decoded input, or of
  ``tone_mapped_input`` of it, in every value.  No float image exists at any point.  ``staged`` as in
  ``retouch_batch_raw``; ``dtype`` is the storage dtype the pictures are those of."""
  from . import _cabi
  if code not in INPUT_CODES:
    raise ValueError('code must be one of %s' % (tuple(INPUT_CODES),))
  raws = list(raws)
  n = len(raws)
  if n == 0:
    raise ValueError('input_pictures_raw: no images')
  if not (linear or tone_mapped):
    raise ValueError('input_pictures_raw: nothing requested (linear and tone_mapped both False)')
  dev = torch.device(device)
  want = [name for name, on in (('linear', linear), ('tone_mapped', tone_mapped)) if on]
  pics = {name: [None] * n for name in want}
  for idx, cs, tables, stride, _k in (stage_raws(raws, dtype, dev) if staged is None else staged):
    luts = dict(zip(('linear', 'tone_mapped'), input_luts(tables, stride, _cabi.codes_max_ragged(cs), code)))
    for name in want:
      lut = torch.from_numpy(luts[name]).to(dev)
      outs = [torch.empty((c.shape[0], c.shape[1], 3), dtype=lut.dtype, device=dev) for c in cs]
      _cabi.codes_lut_ragged(cs, lut, lut.shape[1], outs)
      for i, o in zip(idx, outs):
        pics[name][i] = o
  return tuple(pics[name] for name in want)


def load_agent_weights(agent, state):
  """Accepts an ``Agent`` state dict, a ``GAN.state_dict()`` (keys prefixed 'generator.' / 'critic.' / 'value.') or the
  ``{'model': GAN.state_dict(), 'optim': ...}`` file that ``python -m exposure_amd.train --save`` writes: the
  generator's entries are picked out and the prefix stripped."""
  if 'model' in state and isinstance(state['model'], dict):
    state = state['model']
  if any(k.startswith('generator.') for k in state):
    state = {k[len('generator.'):]: v for k, v in state.items() if k.startswith('generator.')}
  agent.load_state_dict(state)
  return agent


def save_png(path, img):
  """``show_and_save`` of ``net.py:769-772``: ``cv2.imwrite(path, img[:, :, ::-1] * 255.0)`` -- 8 bits per channel,
  rounded to nearest (half to even, as ``cvRound``) and saturated; the file holds RGB."""
  from PIL import Image
  a = np.asarray(img, dtype=np.float32)
  Image.fromarray(np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8), 'RGB').save(path)
  return path


def save_png_u8(path, img_u8):
  """An (H, W, 3) uint8 array of ``save_png``'s encoding (``encode_u8``, or an EXPO_TAP_U8 tap) written as it is."""
  from PIL import Image
  Image.fromarray(np.ascontiguousarray(img_u8), 'RGB').save(path)
  return path


PNG_FILTERS = ('none', 'sub', 'up', 'average', 'paeth', 'adaptive')  # the row filters of encode_png_batch (_cabi.PNG_FILTERS)


def encode_png_batch(pictures, filter='adaptive'):
  """The 8-bit PNG files of (H_i, W_i, 3) uint8 device pictures (``encode_u8``, EXPO_TAP_U8 taps, ``input_pictures_raw``)
  as ``bytes``, encoded on the device in one ragged call (``expo_png_encode_ragged``: the row filter and a Huffman-only
  deflate; the pixels ``save_png_u8`` would write, in a larger file).  The download of the files' lengths is the only
  synchronise; then the used prefix of every buffer is copied out."""
  from . import _cabi
  pictures = [p.contiguous() for p in pictures]
  if not pictures:
    return []
  outs, sizes = _cabi.png_encode_ragged(pictures, filter)
  return [o[:n].cpu().numpy().tobytes() for o, n in zip(outs, sizes.cpu().tolist())]


def save_png_bytes(path, data):
  """A finished PNG file (``encode_png_batch``) written as it is."""
  with open(path, 'wb') as fh:
    fh.write(data)
  return path


JPEG_SUBSAMPLING = ('444', '420')  # the samplings of encode_jpeg_batch (_cabi.JPEG_SUBSAMPLING)


def encode_jpeg_batch(pictures, quality=90, subsampling='420'):
  """The baseline JPEG files of (H_i, W_i, 3) uint8 device pictures (``encode_u8``, EXPO_TAP_U8 taps,
  ``input_pictures_raw``) as ``bytes``, encoded on the device in one ragged call (``expo_jpeg_encode_ragged``, DESIGN.md
  3.34) into buffers of 629 + H W 3 bytes.  The download of the files' lengths is the only synchronise; then the used
  prefix of every buffer is copied out.  A file longer than its buffer (noise at quality 100) is not written by that
  call: those pictures are encoded once more, in one call, into buffers of the reported lengths."""
  from . import _cabi
  pictures = [p.contiguous() for p in pictures]
  if not pictures:
    return []
  outs, sizes = _cabi.jpeg_encode_ragged(pictures, quality, subsampling)
  sizes = sizes.cpu().tolist()
  files = [o[:n].cpu().numpy().tobytes() if n <= o.numel() else None for o, n in zip(outs, sizes)]
  again = [i for i, f in enumerate(files) if f is None]
  if again:
    outs, _ = _cabi.jpeg_encode_ragged([pictures[i] for i in again], quality, subsampling,
                                       capacity=[sizes[i] for i in again])
    for i, o in zip(again, outs):
      files[i] = o[:sizes[i]].cpu().numpy().tobytes()
  return files


def save_tiff_u16(path, img_u16):
  """An (H, W, 3) uint16 array (``encode_u16``, or an EXPO_TAP_U16 tap) as an uncompressed 16-bit RGB TIFF: the file's
  payload is the array byte for byte."""
  from .tiff16 import write_tiff
  write_tiff(path, np.ascontiguousarray(img_u16, dtype=np.uint16))
  return path


def _host_codes(t):
  """A uint8 / uint16 device tensor as a NumPy array (uint16 crosses as int16: the copy of a strided view then needs
  no uint16 kernel of torch)."""
  if t.dtype is torch.uint16:
    return t.view(torch.int16).cpu().numpy().view(np.uint16)
  return t.cpu().numpy()


def tone_mapped_input(linear):
  """``net.py:822-823``: max to white, then gamma 1/2.4 -- the ``input_tone_mapped`` picture of ``GAN.eval``.  Host
  maths also with ``--device-png``: a device ``pow`` cannot be made bit-identical to numpy's.  (``input_pictures_raw``
  makes the same picture on the device without one: this expression over the code range, then a gather.)"""
  a = np.asarray(linear, dtype=np.float32)
  return (a / a.max())**(1 / 2.4)


def output_path(out, image_path, many):
  """--out: a directory (existing, or ending in a path separator) receives <name>.retouched.npy per
  image; with one image it may also be the file itself; with several images and a plain name the
  image's stem is inserted so results do not overwrite each other."""
  import os
  base = os.path.basename(image_path)
  if out is None:
    return image_path + '.retouched.npy'
  if os.path.isdir(out) or out.endswith(os.sep):
    os.makedirs(out, exist_ok=True)
    return os.path.join(out, base + '.retouched.npy')
  if not many:
    return out
  root, ext = os.path.splitext(out)
  return '%s.%s%s' % (root, os.path.splitext(base)[0], ext or '.npy')


CLI_DEVICE = 'cuda:0'  # the device main() runs on (the host tests run the CLI against the CPU stand-in of tests/)

FILTER_BY_SHORT_NAME = {'E': 'ExposureFilter', 'G': 'GammaFilter', 'W': 'ImprovedWhiteBalanceFilter',
                        'S+': 'SaturationPlusFilter', 'T': 'ToneFilter', 'Ct': 'ContrastFilter', 'BW': 'WNBFilter',
                        'C': 'ColorFilter'}


def main(argv=None):
  """``python -m exposure_amd.evaluate [--filters E,G] [--weights w.pt | --tf-checkpoint dir] [--out dir|file] img ...`` -- the
  tensor part of ``evaluate.py:8-31`` / ``GAN.eval`` (``net.py:711-821``): per image, load (16-bit TIFF or
  8-bit sRGB), 5 retouching steps on the GPU, write the linear result.  With ``--batch N`` the images go through
  ``retouch_batch`` in groups of up to N (same files and records).  Returns one record per image."""
  import argparse
  import numpy as np
  from . import filters as F
  from .agent import Agent
  from .config import make_cfg
  ap = argparse.ArgumentParser()
  ap.add_argument('images', nargs='+')
  ap.add_argument('--weights', default=None,
                  help='torch state_dict of exposure_amd.agent.Agent, or the GAN state dict train.py --save writes '
                  '(random init if absent)')
  ap.add_argument('--tf-checkpoint', default=None, metavar='MODEL_DIR',
                  help="directory of a TF-1 checkpoint of the reference (models/<cfg>/<name>): restores "
                  "MODEL_DIR/model.ckpt-<--ckpt> like evaluate.py:27-28 (no TensorFlow needed)")
  ap.add_argument('--ckpt', default='20000', help='checkpoint iteration for --tf-checkpoint (evaluate.py:28: 20000)')
  ap.add_argument('--out', default=None, help='output file (one image) or directory; default <image>.retouched.npy')
  ap.add_argument('--png', action='store_true',
                  help="also write <output>.png (8-bit, the reference's `<name>.retouched.png`, net.py:769-772, 832) "
                  'and, with --show-input, <output>.input_tone_mapped.png (net.py:822-829)')
  ap.add_argument('--show-input', action='store_true')
  ap.add_argument('--show-linear', action='store_true',
                  help="also write <output>.linear.png, the 8-bit picture of the linear input (GAN.eval's `linear`, "
                  'net.py:825-839); wherever --show-input works')
  ap.add_argument('--device-input-png', action='store_true',
                  help="make --show-input's and --show-linear's pictures on the GPU from the integer codes "
                  '(input_pictures_raw): the host evaluates its own expressions on the code range, the device gathers; the '
                  'same PNG bytes as the host path, without the float download and the full-size pow.  Implies '
                  '--device-decode; the pictures are 8-bit PNGs, also with --tiff16')
  ap.add_argument('--step-by-step', action='store_true',
                  help="also write <output>.intermediateNN.png, the picture after every step but the last (evaluate.py:31, "
                  'net.py:820-823); implies --png.  The fused paths write them from the same pass as 8-bit values')
  ap.add_argument('--dtype', default='f16', choices=['f16', 'f32'])
  ap.add_argument('--filters', default=None,
                  help="cfg.filters as comma-separated short names, e.g. 'E,G' (BASELINE config 1); default: all 8")
  ap.add_argument('--seed', type=int, default=None, help='seeds the random-init weights / dropout / noise')
  ap.add_argument('--stepwise', action='store_true', help="the reference's schedule: filter the full-resolution "
                  'tensor at every step instead of one fused pass at the end')
  ap.add_argument('--masking', action='store_true',
                  help="cfg.masking: every filter acts through the reference's spatial mask (filters.py:110-148); the "
                  "heads' shapes do not depend on it.  The reference's schedule unless --fused-masks is given")
  ap.add_argument('--fused-masks', action='store_true',
                  help='with --masking: apply the masked steps in the one fused pass (fp32 between steps, taps, --batch '
                  'in one ragged launch) instead of step by step.  --stepwise wins over it')
  ap.add_argument('--curve-steps', type=int, default=None, metavar='L',
                  help='cfg.curve_steps, 1..16 (default 8): the knots of the Tone and Color curves, which sets the '
                  "shapes of their heads -- weights trained with another L do not load.  L != 8 runs the reference's "
                  'schedule on the generic kernels unless --fused-curves is given')
  ap.add_argument('--fused-curves', action='store_true',
                  help='with --curve-steps L != 8: apply the steps in the one fused pass for any L (fp32 between steps, '
                  'taps, --batch in one ragged launch) instead of step by step.  Not with --stepwise; --masking keeps '
                  'the stepwise schedule; no effect with 8-step curves')
  ap.add_argument('--curve-dispatch', action='store_true',
                  help="with --curve-steps L != 8: the agent's own 64x64 step on the per-image dispatch kernels for any L "
                  '(Agent.curve_dispatch) instead of running every filter on the whole batch; with or without '
                  '--fused-curves; --masking keeps the stack-and-select step; no effect with 8-step curves')
  ap.add_argument('--batch', type=int, default=1, metavar='N',
                  help='retouch up to N images at once, of any sizes, grouped in argument order (retouch_batch: the '
                  'agent runs on the stacked proxies, one ragged launch applies the filters).  z and the dropout '
                  'masks are drawn per batch, so --seed with --batch N does not reproduce --batch 1; with --stepwise '
                  'every image runs alone')
  ap.add_argument('--device-decode', action='store_true',
                  help='read the images as integer codes (load_raw) and linearise them on the GPU, one ragged call per '
                  'group of --batch images (decode_images): the same tensors as the default host decode')
  ap.add_argument('--device-jpeg-decode', action='store_true',
                  help='decode baseline JPEG inputs on the device from the bytes of the files (DESIGN.md 3.35): the same '
                  'codes as PIL, bit for bit, so every output is byte-identical; a file the device decoder does not '
                  'take (progressive, CMYK, not a .jpg) goes through PIL and is named on stderr.  Implies --device-decode')
  ap.add_argument('--jpeg-serial-entropy', action='store_true',
                  help='with --device-jpeg-decode: walk a file without restart markers with one lane instead of a lane per '
                  'subsequence (DESIGN.md 3.36), for comparison runs; the same codes, so every output is byte-identical')
  ap.add_argument('--device-proxy', action='store_true',
                  help="make the agent's 64x64 proxies with one HIP launch per group of --batch images "
                  '(make_low_res_batch) instead of torch\'s interpolate per image.  Same definition, every float32 '
                  'operation rounded on its own: a proxy value can differ from the default path\'s in the last place, '
                  'which in rare cases changes an argmax and with it the chosen filters')
  ap.add_argument('--fused-decode', action='store_true',
                  help='retouch straight from the integer codes (retouch_batch_raw): per group of --batch images the '
                  'device gets the codes as the files hold them, the proxies and the one fused pass gather from the '
                  "images' tables as they load, and the decoded float input is never made.  The same files and records "
                  'as --device-decode --device-proxy, which it implies.  Not with --stepwise or --masking; '
                  '--show-input / --show-linear need --device-input-png (the host pictures need the float input)')
  ap.add_argument('--fused-decode-curves', action='store_true',
                  help='--fused-decode for any --curve-steps: with L != 8 the one pass from the integer codes is the '
                  'one for any L (retouch_batch_raw with curves=\'fused\'), so it is --fused-decode --fused-curves in '
                  'one switch, and writes the same files and records as --device-decode --device-proxy --fused-curves.  '
                  'With 8-step curves it is --fused-decode.  Not with --stepwise or --masking; goes with everything '
                  '--fused-decode goes with')
  ap.add_argument('--pictures-only', action='store_true',
                  help='write no .npy: only the pictures (needs --device-png, --tiff16 or --score); the record\'s '
                  'output is None.  With --fused-decode the float output is not even allocated (outputs=False)')
  ap.add_argument('--device-png', action='store_true',
                  help='write <output>.png from 8-bit values made on the GPU: on the fused paths a tap of the last step '
                  'from the pass that writes the output, with --stepwise an encode of the result.  The same pixels as '
                  '--png, which it implies; --show-input\'s picture keeps its host maths')
  ap.add_argument('--device-png-encode', action='store_true',
                  help='encode every 8-bit PNG that is written from a device picture on the GPU (encode_png_batch: row '
                  'filter and Huffman-only deflate, no LZ77 matches), one call per group of --batch images and kind: '
                  '<output>.png, the --step-by-step intermediates and the --device-input-png pictures.  Valid PNG with '
                  'the same pixels and file names, larger files than the default host compressor\'s (about 1.1 to 1.4 '
                  'times on photographs).  Measured 60 to 340 times faster than PIL to host bytes (DESIGN.md 3.29).  '
                  'Implies --device-png; not with --tiff16')
  ap.add_argument('--png-filter', default='adaptive', choices=list(PNG_FILTERS),
                  help='the row filter of --device-png-encode: one type for every row, or adaptive (per row the type '
                  'with the smallest sum of absolute residuals, libpng\'s heuristic)')
  ap.add_argument('--device-jpeg-encode', action='store_true',
                  help='write a baseline JPEG, encoded on the GPU (encode_jpeg_batch: transform, quantisation and the '
                  'standard Huffman code in independent restart intervals, DESIGN.md 3.34), for every picture for which '
                  '--device-png-encode writes a PNG, under the same name with .jpg: <output>.jpg, the --step-by-step '
                  'intermediates and the --device-input-png pictures, one call per group of --batch images and kind; the '
                  'records list them under jpeg.  Implies --device-png; not with --device-png-encode or --tiff16')
  ap.add_argument('--jpeg-quality', type=int, default=90, metavar='Q',
                  help='the quality of --device-jpeg-encode, 1..100 (libjpeg\'s scaling of the Annex K tables)')
  ap.add_argument('--jpeg-subsampling', default='420', choices=list(JPEG_SUBSAMPLING),
                  help='the chroma sampling of --device-jpeg-encode: 444 or 420')
  ap.add_argument('--tiff16', action='store_true',
                  help='write the pictures as 16-bit RGB TIFFs (uncompressed, little-endian) instead of 8-bit PNGs: '
                  '<output>.tif and, with --step-by-step, <output>.intermediateNN.tif, code = round(value * 65535) '
                  'saturated.  On the fused paths the codes are taps of the pass that writes the output, with --stepwise '
                  'an encode of the results.  With --dtype f16 a value is rounded to fp16 storage first, so the picture '
                  "carries fp16's 11 significant bits: the full 16-bit depth needs --dtype f32.  Not with --png, "
                  '--device-png or --score (8-bit pictures: one pass makes one kind); --show-input keeps its 8-bit PNG')
  ap.add_argument('--score', default=None, metavar='TARGET_DIR',
                  help="after the run, score the retouched pictures against the 8-bit pictures of TARGET_DIR with the "
                  "paper's metric (histogram intersection of luminance, contrast and saturation, exposure_amd.metrics) "
                  'on the GPU: the pictures of --device-png, which it implies, stay on the device and no PNG is read '
                  'back.  Prints the two lines of histogram_intersection.py and appends dict(score, average) to the '
                  'returned records')
  ap.add_argument('--score-seed', type=int, default=None, metavar='N',
                  help="seeds the metric's random crops (default: a different sample every run, as the script)")
  args = ap.parse_args(argv)
  dev = torch.device(CLI_DEVICE)
  if args.seed is not None:
    torch.manual_seed(args.seed)
  flt = None
  if args.filters:
    flt = [getattr(F, FILTER_BY_SHORT_NAME[name.strip()]) for name in args.filters.split(',')]
  cfg = make_cfg(filters=flt)
  if args.masking:
    cfg.masking = True
  if args.curve_steps is not None:
    if not 1 <= args.curve_steps <= 16:
      ap.error('--curve-steps must be in 1..16')
    cfg.curve_steps = args.curve_steps
  if args.fused_decode_curves and args.stepwise:
    ap.error('--fused-decode-curves does not go with --stepwise: the pass from codes is the fused one')
  if args.fused_decode_curves:
    args.fused_decode = args.fused_curves = True
  if args.fused_curves and args.stepwise:
    ap.error('--fused-curves does not go with --stepwise: they are two schedules of the full-resolution pass')
  agent = Agent(cfg).to(dev)
  agent.curve_dispatch = bool(args.curve_dispatch)
  if args.weights and args.tf_checkpoint:
    ap.error('--weights and --tf-checkpoint are alternatives')
  if args.weights:
    load_agent_weights(agent, torch.load(args.weights, map_location=dev))
  if args.tf_checkpoint:
    from . import checkpoint
    checkpoint.restore(agent, args.tf_checkpoint, args.ckpt)
  dt = torch.float16 if args.dtype == 'f16' else torch.float32
  if args.batch < 1:
    ap.error('--batch must be >= 1')
  if args.device_jpeg_encode and (args.device_png_encode or args.tiff16):
    ap.error('--device-jpeg-encode does not go with --device-png-encode or --tiff16: a picture is written once')
  if not 1 <= args.jpeg_quality <= 100:
    ap.error('--jpeg-quality must be in 1..100')
  if args.tiff16 and (args.png or args.device_png or args.score or args.device_png_encode):
    ap.error('--tiff16 does not go with --png, --device-png, --device-png-encode or --score: they need the 8-bit '
             'pictures, and one pass makes pictures of one depth')
  if args.device_png_encode or args.device_jpeg_encode:
    args.device_png = True
  if args.score:
    args.device_png = True
  if args.fused_decode:
    if any(f.uses_generic_kernels() for f in agent.filters) and not args.fused_decode_curves:
      ap.error('--fused-decode needs 8-step curves: the pass from codes for --curve-steps %d is '
               '--fused-decode-curves' % cfg.curve_steps)
    if args.stepwise or args.masking or ((args.show_input or args.show_linear) and not args.device_input_png):
      ap.error('%s does not go with --stepwise, --masking or --show-input: the pass from codes is the unmasked fused '
               'one, and the tone-mapped picture needs the float input'
               % ('--fused-decode-curves' if args.fused_decode_curves else '--fused-decode'))
    args.device_decode = args.device_proxy = True
  if args.device_input_png or args.device_jpeg_decode:
    args.device_decode = True
  if args.pictures_only and not (args.device_png or args.tiff16):
    ap.error('--pictures-only needs --device-png, --tiff16 or --score: it writes the pictures the device makes')
  if (args.step_by_step and not args.tiff16) or args.device_png:
    args.png = True
  proxy = 'device' if args.device_proxy else 'torch'
  code = 'u16' if args.tiff16 else 'u8'
  inter_kind = code if args.step_by_step else None
  picture = 'u16' if args.tiff16 else args.device_png  # the pictures retouch makes on the device
  masks = 'fused' if args.fused_masks else 'stepwise'
  curves = 'fused' if args.fused_curves else 'stepwise'
  records = []
  pictures = []  # --score: every emitted image's uint8 picture, kept on the device (not the float outputs)

  show = [name for name, on in (('linear', args.show_linear), ('input_tone_mapped', args.show_input)) if on]

  def input_pictures(raws, staged=None):
    """--device-input-png: per image the requested input pictures as uint8 device tensors, by name (else None)"""
    if not (args.device_input_png and show):
      return None
    made = input_pictures_raw(raws, dt, dev, linear=args.show_linear, tone_mapped=args.show_input, staged=staged)
    return [dict(zip(show, per)) for per in zip(*made)]

  def encode_group(pics, inters, inps):
    """--device-png-encode, --device-jpeg-encode: per image of a group its finished PNG (JPEG) files by name, one
    device call per kind (the retouched pictures, the intermediates, the input pictures)"""
    if args.device_jpeg_encode:
      encode = lambda pictures: encode_jpeg_batch(pictures, args.jpeg_quality, args.jpeg_subsampling)
    else:
      encode = lambda pictures: encode_png_batch(pictures, args.png_filter)
    files = [dict() for _ in pics]
    for i, data in enumerate(encode(pics)):
      files[i]['retouched'] = data
    if inters is not None:
      keys = [(i, s) for i, inter in enumerate(inters) for s in range(inter.shape[0])]
      for (i, s), data in zip(keys, encode([inters[i][s] for i, s in keys])):
        files[i]['intermediate%02d' % s] = data
    if inps:
      keys = [(i, name) for i in range(len(pics)) for name in show]
      for (i, name), data in zip(keys, encode([inps[i][name] for i, name in keys])):
        files[i][name] = data
    return files

  def save_picture(path, key, files, tensor):
    """an 8-bit device picture as a PNG: the file the device encoded (with --device-jpeg-encode a JPEG, under the
    same name with .jpg), or PIL's of the downloaded values"""
    if files is not None and key in files:
      return save_png_bytes(path[:-4] + '.jpg' if args.device_jpeg_encode else path, files[key])
    return save_png_u8(path, tensor.cpu().numpy())

  def save_input_pngs(pngs, stem, hi, inp, files=None):
    for name in show:
      if inp is not None:
        pngs[name] = save_picture('%s.%s.png' % (stem, name), name, files, inp[name])
      else:
        a = hi[0].float().cpu().numpy()
        pngs[name] = save_png('%s.%s.png' % (stem, name), tone_mapped_input(a) if name == 'input_tone_mapped' else a)

  def emit(path, hi, out, states, ops, inter=None, pic=None, inp=None, files=None):
    """print, save and record one image's result (hi, out: (1, H, W, 3); states, ops: that image's rows; inter: its
    (S-1, H, W, 3) uint8 / uint16 intermediates with --step-by-step; pic: its (H, W, 3) uint8 picture with
    --device-png, uint16 with --tiff16; inp: its input pictures with --device-input-png; files: its device-encoded
    PNG files with --device-png-encode)"""
    trace = ops['selected']
    names = [agent.filters[int(j)].get_short_name() for j in trace[0]]
    print('%s: %dx%d  filters: %s' % (path, hi.shape[2], hi.shape[1], ' '.join(names)))
    dst = output_path(args.out, path, len(args.images) > 1)
    result = None
    if not args.pictures_only:
      result = out[0].float().cpu().numpy()
      np.save(dst, result)
    if args.score:
      pictures.append(pic.contiguous())
    pngs, tiffs = {}, {}
    stem = dst[:-4] if dst.endswith('.npy') else dst
    if args.tiff16:
      tiffs['retouched'] = save_tiff_u16(stem + '.tif', _host_codes(pic))
      save_input_pngs(pngs, stem, hi, inp)
      if inter is not None:
        for i, a in enumerate(_host_codes(inter)):
          tiffs['intermediate%02d' % i] = save_tiff_u16('%s.intermediate%02d.tif' % (stem, i), a)
    if args.png:
      if pic is not None:
        pngs['retouched'] = save_picture(stem + '.png', 'retouched', files, pic)
      else:
        pngs['retouched'] = save_png(stem + '.png', result)
      save_input_pngs(pngs, stem, hi, inp, files)
      if inter is not None and files is not None:
        for i in range(inter.shape[0]):
          pngs['intermediate%02d' % i] = save_picture('%s.intermediate%02d.png' % (stem, i), 'intermediate%02d' % i, files, None)
      elif inter is not None:
        for i, a in enumerate(inter.cpu().numpy()):
          pngs['intermediate%02d' % i] = save_png_u8('%s.intermediate%02d.png' % (stem, i), a)
    records.append(dict(image=path, output=None if args.pictures_only else dst, png=pngs, tiff=tiffs, filters=names, states=states[0].cpu().tolist(),
                        abi_filter_ids=ops['abi_filter_ids'][0].cpu().tolist(),
                        params24=ops['params24'][0].cpu().numpy()))
    if args.device_jpeg_encode:  # the files the device encoded are JPEGs: listed under their own key
      records[-1]['jpeg'] = {k: v for k, v in pngs.items() if files is not None and k in files}
      records[-1]['png'] = {k: v for k, v in pngs.items() if k not in records[-1]['jpeg']}

  def load(path):
    return torch.from_numpy(np.ascontiguousarray(load_image(path))).to(dev).to(dt)[None]

  def load_group(paths):
    """-> the images, and per image its device-made input pictures (None without --device-input-png)"""
    if args.device_decode:
      raws = load_raws(paths, dev, args.device_jpeg_decode, False if args.jpeg_serial_entropy else 'auto')
      if args.device_input_png and show:  # the codes go up once, for the decode and for the input pictures
        staged = list(stage_raws(raws, dt, dev))
        return decode_images(raws, dt, dev, staged), input_pictures(raws, staged)
      return decode_images(raws, dt, dev), None
    return [load(path) for path in paths], None

  def emit_batch(paths, his, res, inps=None):
    outs, states, ops = res[0], res[2], res[3]
    files = encode_group(list(res[-1]), list(res[4]) if inter_kind else None, inps) if encode_files else None
    for i, (path, hi, out) in enumerate(zip(paths, his, outs)):
      emit(path, hi, out, states[i:i + 1], {k: v[i:i + 1] for k, v in ops.items()}, res[4][i] if inter_kind else None,
           res[-1][i] if picture else None, inps[i] if inps else None, files[i] if files else None)

  encode_files = args.device_png_encode or args.device_jpeg_encode
  if args.fused_decode:  # also with --batch 1: groups of one image
    for b in range(0, len(args.images), args.batch):
      paths = args.images[b:b + args.batch]
      raws = load_raws(paths, dev, args.device_jpeg_decode, False if args.jpeg_serial_entropy else 'auto')
      staged = list(stage_raws(raws, dt, dev))  # the codes go up once, for the pass and for the input pictures
      res = retouch_batch_raw(agent, raws, dt, dev, return_trace='full', intermediates=inter_kind, picture=picture,
                              outputs=not args.pictures_only, staged=staged, curves=curves)
      # emit reads of `hi` its size alone here (the input pictures come from the codes): the codes have it
      emit_batch(paths, [codes[None] for codes, _kind in raws], res, input_pictures(raws, staged))
  elif args.batch == 1 or args.stepwise:
    for path in args.images:
      (hi,), inps = load_group([path])
      res = retouch(agent, hi, return_trace='full', fused=not args.stepwise, intermediates=inter_kind, proxy=proxy,
                    picture=picture, masks=masks, curves=curves)
      inter = res[4][:, 0] if inter_kind else None
      files = encode_group([res[-1][0]], [inter] if inter_kind else None, inps) if encode_files else None
      emit(path, hi, res[0], res[2], res[3], inter, res[-1][0] if picture else None, inps[0] if inps else None,
           files[0] if files else None)
  else:
    for b in range(0, len(args.images), args.batch):
      paths = args.images[b:b + args.batch]
      his, inps = load_group(paths)
      res = retouch_batch(agent, his, return_trace='full', intermediates=inter_kind, proxy=proxy,
                          picture=picture, masks=masks, curves=curves)
      emit_batch(paths, his, res, inps)
  if args.score:
    import random
    from . import metrics
    rng = random.Random(args.score_seed) if args.score_seed is not None else None
    ints, avg = metrics.score(metrics.set_statistics(pictures, rng, names=args.images),
                              metrics.read_statistics(args.score, rng=rng, device=dev))
    for line in metrics.format_score(ints, avg):
      print(line)
    records.append(dict(score=ints, average=avg))
  return records


if __name__ == '__main__':
  main()
