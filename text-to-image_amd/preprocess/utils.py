"""The reference's preprocess/utils.py restated on NumPy and Pillow's decoder: the host statement of the load-size image
transform, which the tests hold to Pillow itself and the device path (kernels.preprocess_images) to it.

Per image the reference computes `scipy.misc.imresize(colorize(imread(path))[crop], [S, S], 'bicubic')` on a FLOAT image.
SciPy removed imread / imresize; what they did is:
  imread     PIL.Image.open + np.array (palette images converted to RGB / RGBA, 1-bit images to 8-bit grey), as float64;
  colorize   a 2-D image becomes three equal channels, a 4-channel image keeps its first three;
  custom_crop   a square of half-side int(max(w, h) * 0.75) around the box centre, cut at the image's borders (`crop_box`);
  imresize   scipy's bytescale over the whole cropped image in float64 — a per-image contrast stretch, min -> 0 and max -> 255,
             a constant image comes out black — then PIL's Image.resize((S, S), BICUBIC) on the uint8 result.
Because the float64 image only ever holds the integers 0 .. 255, bytescale is a 256-entry table per image (`bytescale_lut`); the
resize is evaluation/resize.py's resize_u8_bicubic.  This path is slow (tens of ms per image) and is only the checker.

Two things the reference gets silently wrong or crashes on are refused here, by name: an empty crop (a box outside the image)
and an image or crop with a side of exactly 3 or 4 pixels (scipy's toimage then takes that axis for the channels)."""
import os

import numpy as np

from ..evaluation.resize import resize_u8_bicubic


def imread_u8(path):
    """scipy.misc.imread before its float cast: uint8 [H, W], [H, W, 3] or [H, W, 4]."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode == 'P':
            im = im.convert('RGBA' if 'transparency' in im.info else 'RGB')
        elif im.mode == '1':
            im = im.convert('L')
        img = np.array(im)
    if img.ndim == 0:
        raise ValueError('%s: the decoder returned a scalar, not an image' % path)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
        raise ValueError('%s: unsupported image (%s %s); 8-bit grey, RGB or 4-channel images only' % (path, img.dtype, img.shape))
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    return img


def imread(path):
    return imread_u8(path).astype(np.float64)


def colorize(img):
    """-> [H, W, 3]: grey is repeated over three channels, a fourth channel is dropped."""
    img = np.asarray(img)
    if img.ndim == 2:
        return np.repeat(img[..., None], 3, axis=2)
    return img[..., :3] if img.shape[2] == 4 else img


def crop_box(shape, bbox):
    """custom_crop's rectangle for an image of `shape` [height, width, ...] and bbox = [x-left, y-top, width, height] (cast to
    int, as the reference's load_bbox does) -> (y1, y2, x1, x2).  May be empty (y2 <= y1 or x2 <= x1): see check_crop."""
    x, y, w, h = (int(v) for v in bbox)
    center_x = int((2 * x + w) / 2)
    center_y = int((2 * y + h) / 2)
    R = int(max(w, h) * 0.75)
    y1 = max(0, center_y - R)
    y2 = min(int(shape[0]), center_y + R)
    x1 = max(0, center_x - R)
    x2 = min(int(shape[1]), center_x + R)
    return y1, y2, x1, x2


def check_crop(shape, box, name='image'):
    """Refuses what the reference gets wrong: box = (y1, y2, x1, x2) of an image of `shape`; `name` goes into the message."""
    y1, y2, x1, x2 = box
    if y2 <= y1 or x2 <= x1:
        raise ValueError('%s: the crop rows %d:%d, columns %d:%d of the %dx%d image is empty (bounding box outside the image)'
                         % (name, y1, y2, x1, x2, shape[0], shape[1]))
    if (y2 - y1) in (3, 4) or (x2 - x1) in (3, 4):
        raise ValueError('%s: a side of exactly 3 or 4 pixels (%dx%d) is refused: scipy.misc.imresize takes that axis for the '
                         'channels' % (name, y2 - y1, x2 - x1))
    return box


def custom_crop(img, bbox):
    y1, y2, x1, x2 = crop_box(img.shape, bbox)
    return img[y1:y2, x1:x2, :]


def bytescale_lut(cmin, cmax):
    """scipy's bytescale of the values 0 .. 255 for an image whose min / max are cmin / cmax, in float64 -> uint8 [256]."""
    cmin, cmax = float(cmin), float(cmax)
    cscale = cmax - cmin
    if cscale == 0:
        cscale = 1.0
    scale = 255.0 / cscale
    u = np.arange(256, dtype=np.float64)
    return (np.clip((u - cmin) * scale, 0, 255) + 0.5).astype(np.uint8)


def transform(image, image_size, is_crop, bbox, name='image'):
    """image: what imread returns (float or uint8, holding integers 0 .. 255) -> uint8 [image_size, image_size, 3]."""
    image = colorize(np.asarray(image))
    box = crop_box(image.shape, bbox) if is_crop else (0, image.shape[0], 0, image.shape[1])
    y1, y2, x1, x2 = check_crop(image.shape, box, name)
    image = image[y1:y2, x1:x2, :]
    u8 = image.astype(np.uint8)
    if not np.array_equal(u8, image):
        raise ValueError('%s: transform expects the integers 0 .. 255 (a decoded 8-bit image)' % name)
    lut = bytescale_lut(u8.min(), u8.max())
    return resize_u8_bicubic(lut[u8], image_size, image_size)


def get_image(image_path, image_size, is_crop=False, bbox=None):
    return transform(imread(image_path), image_size, is_crop, bbox, name=image_path)


def mkdir_p(path):
    """`mkdir -p`: an existing directory is fine, an existing file of that name is an error."""
    os.makedirs(path, exist_ok=True)
