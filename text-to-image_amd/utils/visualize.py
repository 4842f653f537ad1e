"""Caption visualiser helpers — the role of the reference's utils/visualize.py, restated from its behaviour.

Interpolations in the noise and embedding spaces, captioned sample sheets and the closest-neighbour sheet.  Differences
from the reference, all deliberate:
  - a generator is a callable `gen(z, cond) -> images [B,h,w,3]` instead of a TF session plus an op and placeholder names;
  - the closest-neighbour search is one launch of `kernels.nearest_images` over the resident uint8 store instead of a
    Python loop of `next_batch_test(1, idx, 1)` + float64 `np.linalg.norm` per train image and per generated image; the
    crop table is drawn in that loop's order from the same generators, so equal seeds give equal crops;
  - PNGs are written with Pillow (scipy.misc is gone), and when none of the reference's three font files exists the
    caption is drawn with Pillow's built-in scalable font.
Kept from the reference on purpose: `slerp(a, b, 1) = b` but `lerp(a, b, 1) = a`, so the noise sheet runs from z[1] to z[0]
while the embedding sheet runs from cond1 to cond2; `get_interpolated_batch` has 7 entries for a batch of 6 (its float
`arange` overshoots); sheets show 8 images per row under a white caption row."""
import os

import numpy as np
import torch

from .. import kernels as K
from .utils import denormalize_images

FONT_PATHS = ('/Library/Fonts/Arial.ttf', 'arial.ttf', '/usr/share/fonts/truetype/freefont/FreeMono.ttf')
NEIGHBOUR_TEXT = 'Generated images and their closest neighbours'


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _check_miu(miu):
    if miu < 0 or miu > 1:
        raise ValueError('miu must be in [0, 1] but it is %r' % (miu,))


def slerp(a, b, miu):
    """Spherical interpolation: a at miu = 0, b at miu = 1."""
    _check_miu(miu)
    if miu == 0:
        return a
    if miu == 1:
        return b
    cos = np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b))
    omega = np.arccos(cos)
    return (np.sin((1.0 - miu) * omega) * a + np.sin(miu * omega) * b) / np.sin(omega)


def lerp(a, b, miu):
    """Linear interpolation weighted the reference's way round: a at miu = 1, b at miu = 0."""
    _check_miu(miu)
    return miu * a + (1. - miu) * b


def get_interpolated_batch(a, b, batch_size=64, method='slerp'):
    """Interpolations at miu = 1, 1 - 1/bs, ... (a float arange down to just above 0) and then at miu = 0.  That is bs
    entries when 1/bs is exact in binary and can be one more otherwise (7 for bs = 6)."""
    fn = {'slerp': slerp, 'lerp': lerp}.get(method)
    if fn is None:
        return []
    step = 1 / batch_size
    return [fn(a, b, miu) for miu in np.arange(1.0, step, -step)] + [fn(a, b, 0.0)]


def preprocess_caption(cap):
    """First letter upper case, a full stop at the end (an empty caption stays empty)."""
    if not cap:
        return cap
    cap = cap[:1].upper() + cap[1:]
    return cap if cap.endswith('.') else cap + '.'


preporcess_caption = preprocess_caption        # the reference's spelling


def _font(font_size):
    from PIL import ImageFont
    for path in FONT_PATHS:
        try:
            return ImageFont.truetype(path, font_size)
        except OSError:
            pass
    return ImageFont.load_default(font_size)


def write_caption(img, caption, font_size, vert_pos, split=50):
    """Draws `caption` in black at (2, vert_pos) of a uint8 image; a caption with a space at or after character `split` is
    broken there onto a second line one font size lower.  -> new uint8 array."""
    from PIL import Image, ImageDraw
    pil = Image.fromarray(img)
    draw = ImageDraw.Draw(pil)
    font = _font(font_size)
    cut = caption.find(' ', split)
    lines = [caption] if cut == -1 else [caption[:cut], caption[cut + 1:]]
    for i, line in enumerate(lines):
        draw.text((2, vert_pos + i * font_size), line, font=font, fill=(0, 0, 0))
    return np.array(pil)


def prepare_img_for_captioning(img_batch, bottom, rows=None):
    """uint8 sheet: a white row, then `rows` rows of min(8, B) images (default B // n), then another white row if `bottom`."""
    img_batch = _host(img_batch)
    B = img_batch.shape[0]
    n = min(8, B)
    h, w, c = img_batch[0].shape
    if rows is None:
        rows = B // n
    white = np.full((h, n * w, c), 255.0)
    images = denormalize_images(img_batch)
    parts = [white]
    for r in range(rows):
        if B > r * n:
            parts.append(np.concatenate([images[i] for i in range(r * n, (r + 1) * n)], axis=1))
    if bottom:
        parts.append(white)
    return np.concatenate(parts, axis=0).astype(np.uint8)


def _save(sheet, path):
    from PIL import Image
    d = os.path.dirname(path)
    if d and not os.path.exists(d):
        os.makedirs(d)
    Image.fromarray(sheet).save(path)


def save_cap_batch(img_batch, caption, path, rows=None, split=50):
    """Sheet of images with `caption` written in the white top row; written to `path` (PNG) and returned."""
    h = _host(img_batch).shape[1]
    sheet = prepare_img_for_captioning(img_batch, bottom=False, rows=rows)
    sheet = write_caption(sheet, preprocess_caption(caption), h // 3 - 2, 10, split=split)
    _save(sheet, path)
    return sheet


def save_interp_cap_batch(img_batch, cap1, cap2, path, rows=None):
    """Sheet of an interpolation: cap1 in the white top row, cap2 in the white bottom row."""
    h = _host(img_batch).shape[1]
    font_size = h // 3 - 2
    sheet = prepare_img_for_captioning(img_batch, bottom=True, rows=rows)
    sheet = write_caption(sheet, preprocess_caption(cap1), font_size, 10)
    sheet = write_caption(sheet, preprocess_caption(cap2), font_size, sheet.shape[0] - h + 10)
    _save(sheet, path)
    return sheet


def _generator_batch(batch, batch_size, what):
    batch = np.asarray(batch, dtype=np.float32)
    if batch.shape[0] != batch_size:
        raise ValueError('%s has %d entries but the generator takes batches of %d (get_interpolated_batch gives %d entries for '
                         'a batch of %d)' % (what, batch.shape[0], batch_size, batch.shape[0], batch_size))
    return batch


def gen_noise_interp_img(gen, cond, z_dim, batch_size):
    """One caption, z slerped between two draws (the sheet runs from the second draw to the first)."""
    z = np.random.standard_normal(size=(2, z_dim))
    sample_z = _generator_batch(get_interpolated_batch(z[0], z[1], batch_size=batch_size, method='slerp'), batch_size,
                                'the interpolated z batch')
    cond = np.tile(_host(cond).reshape(1, -1), (batch_size, 1))
    return gen(sample_z, cond)


def gen_cond_interp_img(gen, cond1, cond2, z_dim, batch_size):
    """Fresh z per image, the embedding lerped from cond1 to cond2."""
    sample_z = np.random.standard_normal(size=(batch_size, z_dim)).astype(np.float32)
    cond = _generator_batch(get_interpolated_batch(_host(cond1), _host(cond2), batch_size=batch_size, method='lerp'), batch_size,
                            'the interpolated embedding batch')
    return gen(sample_z, cond)


def gen_captioned_img(gen, cond, z_dim, batch_size):
    """A batch of images of one caption embedding."""
    sample_z = np.random.standard_normal(size=(batch_size, z_dim)).astype(np.float32)
    cond = np.tile(_host(cond).reshape(1, -1), (batch_size, 1))
    return gen(sample_z, cond)


def stage_imgs_host(samples, size):
    """The host statement of the reference's float `scipy.misc.imresize(img, (size, size), interp='nearest')` before its
    / 127.5 - 1: models/pggan/visualize_last_stage.py's `bytescale` of (img + 1) * 127.5, then Pillow's NEAREST resize.
    samples [n,h,w,C] (C = 1 or 3) -> uint8 [n,size,size,C].  The checker of kernels.bytescale_nearest; nothing on the product
    path calls it."""
    from PIL import Image
    from ..models.pggan.visualize_last_stage import bytescale
    samples = np.asarray(_host(samples), dtype=np.float32)
    C = samples.shape[3]
    out = np.empty((samples.shape[0], size, size, C), np.uint8)
    for i, sample in enumerate(samples):
        u8 = bytescale((np.array(sample) + 1.0) * 127.5)
        if C == 3:
            out[i] = np.array(Image.fromarray(u8).resize((size, size), Image.NEAREST))
        else:               # Pillow has no 1-, 2- or 4-channel image of this meaning: one grey plane at a time (NEAREST mixes no channels)
            for ch in range(C):
                out[i, :, :, ch] = np.array(Image.fromarray(u8[:, :, ch]).resize((size, size), Image.NEAREST))
    return out


def gen_multiple_stage_img(gens, cond, z_dim, batch_size, size=128):
    """One z batch through every generator of `gens` (the stages of one model): the first 8 images of each, NOT clipped (the
    reference does not clip here), resized to size x size as the reference's float imresize(..., 'nearest') does — per image
    bytescale + Pillow NEAREST, one kernels.bytescale_nearest call per generator — then / 127.5 - 1 in float64 on the host, so
    that a sheet's denormalize_images truncates exactly as the reference's.  -> float64 [8 * len(gens), size, size, 3]."""
    sample_z = np.random.standard_normal((batch_size, z_dim))
    out = []
    for gen in gens:
        imgs = gen(sample_z, cond)[:8]
        if not torch.is_tensor(imgs) or not imgs.is_cuda:          # the file's generators hand back host arrays
            imgs = torch.as_tensor(np.asarray(_host(imgs), dtype=np.float32)).to('cuda')
        out.append(K.bytescale_nearest(imgs, size).cpu().numpy() / 127.5 - 1.0)
    return np.concatenate(out)


def closest_images_of_batch(samples, split):
    """Closest image of `split` (a preprocess.dataset.Dataset) to each of the Q samples [Q,s,s,3] (values clipped to [-1, 1]).

    Crop table: what the reference's loop would draw — query q compares with `next_batch_test(1, n, 1)` for n = 0..N-1, one
    crop / flip draw each, so `split._draw_crops(Q*N, S)` with query q owning rows [q*N, (q+1)*N).  A split without
    augmentation compares with whole images and needs S == s.  One `kernels.nearest_images` launch finds the winners; each
    neighbour is materialised with its query's own crop of it.
    -> (neighbours float32 [Q,s,s,3] (device), ids int64 [Q], (row0, col0, flip) int32 [Q,N] each or None, dist2 float64 [Q])"""
    src = split.images
    q = torch.as_tensor(_host(samples), dtype=torch.float32).to(src.device).contiguous()
    Q, s = q.shape[0], q.shape[1]
    N, S = split.num_examples, int(src.shape[1])
    if split._aug_flag:
        if s != split._imsize:
            raise ValueError('samples are %dx%d but the split crops %dx%d images' % (s, s, split._imsize, split._imsize))
        crops = tuple(a.reshape(Q, N) for a in split._draw_crops(Q * N, S))
        dev = [torch.from_numpy(a).to(src.device) for a in crops]
    else:
        if s != S:
            raise ValueError('the split has no augmentation: samples must be %dx%d like its stored images, got %dx%d' % (S, S, s, s))
        crops, dev = None, [None, None, None]
    ids, dist2 = K.nearest_images(src, q, *dev)
    ids_h = ids.cpu().numpy()
    if crops is None:
        r0 = c0 = fl = np.zeros(Q, np.int32)
    else:
        r0, c0, fl = (a[np.arange(Q), ids_h] for a in crops)
    todev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(src.device)
    neighbours = K.crop_flip_normalize(src, todev(ids_h), todev(r0), todev(c0), todev(fl), s)
    return neighbours, ids, crops, dist2


def gen_closest_neighbour_img(gen, cond, z_dim, batch_size, dataset):
    """Generates a batch, keeps its first 8 images clipped to [-1, 1] and finds their closest train images.
    -> (samples, neighbours, ids, crops) — the first two as NumPy float32, then what closest_images_of_batch returns."""
    sample_z = np.random.standard_normal(size=(batch_size, z_dim)).astype(np.float32)
    samples = np.clip(_host(gen(sample_z, cond))[:8], -1., 1.)
    neighbours, ids, crops, _ = closest_images_of_batch(samples, dataset.train)
    return samples, _host(neighbours), ids, crops
