"""Sliced Wasserstein distance (SWD) between Laplacian-pyramid patch descriptors of real and generated images — the metric of
Karras et al., "Progressive growing of GANs" (their sliced_wasserstein.py), one number per resolution level.  The reference has no
such metric; like evaluation/imd.py it is an addition.  Everything heavy runs in csrc/t2i_swd.hip:

  1. Laplacian pyramid of each batch, L = pyramid_levels(side) levels (t2i_laplacian_pyramid): 5 x 5 binomial, scipy 'mirror' edges.
  2. Per image and level, P = `nhoods` neighbourhoods of 7 x 7 x C at integer centres in [3, side - 3), flattened (c, dy, dx) into
     rows of D = 49 C floats of the level's descriptor store [n_images P, D] (t2i_swd_descriptors), one store per side.
  3. Per channel, over all rows and the channel's 49 columns: mean and population standard deviation in fp64
     (t2i_swd_channel_stats), separately for the real and the generated set.  The standardised matrix is never formed:
  4. for each of R = `repeats` repeats, D x `dirs` unit directions; both sets are standardised while they are projected
     (t2i_swd_project) into one [2 dirs, rows_pad] buffer, every slice of which is sorted by one t2i_segmented_sort_f32 call; the
     distance is the mean |pa - pb| over all entries (t2i_sorted_l1_mean).  A level's SWD is the mean over the repeats, x 10^3.

Every random draw comes from the object's own np.random.RandomState(seed) — the global np.random stream, which the evaluators'
reference-order draws depend on, is never touched: per add() and level, the centres of the real batch and then of the generated
batch as randint(3, side - 3, size=(n, P, 2)); in finalize(), per level and repeat, randn(D, dirs), each column normalised to unit
length in float64 and cast to float32."""
import numpy as np
import torch

from .. import kernels as K

MIN_SIDE = 16          # the coarsest pyramid level


def pyramid_levels(side):
    """1 + the number of halvings that keep the side >= 16: 256 -> 5, 64 -> 3, 16 -> 1."""
    side = int(side)
    if side < MIN_SIDE:
        raise ValueError('SWD needs images of at least %d x %d, got a side of %d' % (MIN_SIDE, MIN_SIDE, side))
    levels = 1
    while side % 2 == 0 and side // 2 >= MIN_SIDE:
        side //= 2
        levels += 1
    return levels


def draw_positions(rng, n, nhoods, side):
    """Centres (y, x) of one batch at one level: int32 [n, nhoods, 2] in [3, side - 3)."""
    return rng.randint(3, side - 3, size=(n, nhoods, 2)).astype(np.int32)


def draw_directions(rng, D, dirs):
    """float32 [D, dirs]: randn, every column normalised to unit length in float64."""
    d = rng.randn(D, dirs)
    d /= np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    return d.astype(np.float32)


class SlicedWasserstein(object):
    """SlicedWasserstein((H, W, C), n_images, device): add(real, gen) per batch of device float32 [n, H, W, C] images (any common
    scale: the descriptors are standardised), then finalize() -> dict(levels=[SWD x 10^3 per level, finest first], mean, sides)."""

    def __init__(self, shape, n_images, device, seed=0, nhoods=128, repeats=4, dirs=128, verbose=True):
        H, W, C = (int(s) for s in shape)
        if H != W:
            raise ValueError('SWD needs square images, got %d x %d' % (H, W))
        self.levels = pyramid_levels(H)
        if not 1 <= C <= 4:
            raise ValueError('SWD takes images of 1 to 4 channels, got %d' % C)
        if int(n_images) <= 0 or min(int(nhoods), int(repeats), int(dirs)) <= 0:
            raise ValueError('SWD needs positive n_images, nhoods, repeats and dirs (got %r, %r, %r, %r)' % (n_images, nhoods, repeats, dirs))
        self.shape, self.n_images, self.device = (H, W, C), int(n_images), torch.device(device)
        self.nhoods, self.repeats, self.dirs = int(nhoods), int(repeats), int(dirs)
        self.sides = [H >> i for i in range(self.levels)]
        self.rng = np.random.RandomState(seed)
        self.count = 0
        rows, D = self.n_images * self.nhoods, 49 * C
        nbytes = 2 * self.levels * rows * D * 4
        if verbose:
            print('SWD: %d levels (sides %s), %d descriptors of %d floats per level and side: %d bytes of descriptor stores' % (
                self.levels, self.sides, rows, D, nbytes))
        self.real = [torch.empty((rows, D), dtype=torch.float32, device=self.device) for _ in range(self.levels)]
        self.gen = [torch.empty((rows, D), dtype=torch.float32, device=self.device) for _ in range(self.levels)]

    def add(self, real, gen):
        """One batch of each set: both pyramids, then per level the descriptors of the real and of the generated images."""
        H, W, C = self.shape
        if tuple(real.shape) != tuple(gen.shape) or tuple(real.shape[1:]) != (H, W, C) or real.shape[0] == 0:
            raise ValueError('SWD.add: real %s and gen %s must both be [n, %d, %d, %d]' % (tuple(real.shape), tuple(gen.shape), H, W, C))
        n = int(real.shape[0])
        if self.count + n > self.n_images:
            raise ValueError('SWD.add: %d images more than the %d the stores were sized for' % (self.count + n - self.n_images, self.n_images))
        pr = K.laplacian_pyramid(real.float().contiguous(), self.levels)
        pg = K.laplacian_pyramid(gen.float().contiguous(), self.levels)
        row0 = self.count * self.nhoods
        for i, side in enumerate(self.sides):
            for pyr, store in ((pr, self.real), (pg, self.gen)):
                K.swd_descriptors(pyr[i], draw_positions(self.rng, n, self.nhoods, side), store[i], row0)
        self.count += n

    def _level(self, i):
        rows, C = self.count * self.nhoods, self.shape[2]
        A, B = self.real[i][:rows], self.gen[i][:rows]
        stats = []
        for name, X in (('real', A), ('generated', B)):
            mean, std = K.swd_channel_stats(X, C)
            if not K.is_dry():
                s = std.cpu().numpy()
                if not np.all(s > 0):            # also NaN
                    raise ValueError('SWD: level %d (side %d), channel %d of the %s set has standard deviation %r: its '
                                     'descriptors cannot be standardised' % (i, self.sides[i], int(np.argmin(s > 0)), name, float(s[np.argmin(s > 0)])))
            stats.append((mean, std))
        S = self.dirs
        buf = torch.empty((2 * S, K.next_pow2(rows)), dtype=torch.float32, device=self.device)
        dists = []
        for _ in range(self.repeats):
            d = torch.from_numpy(draw_directions(self.rng, 49 * C, S)).to(self.device)
            K.swd_project(A, stats[0][0], stats[0][1], d, out=buf[:S])
            K.swd_project(B, stats[1][0], stats[1][1], d, out=buf[S:])
            K.segmented_sort(buf)
            dists.append(K.sorted_l1_mean(buf[:S], buf[S:], rows))
        return torch.cat(dists)

    def finalize(self):
        """-> dict(levels: SWD x 10^3 per level, finest first; mean: their mean; sides: the levels' image sides)."""
        if self.count == 0:
            raise ValueError('SWD.finalize: no images were added')
        per_level = [self._level(i) for i in range(self.levels)]                 # float64 [repeats] each, on the device
        levels = [float(np.mean(d.cpu().numpy()) * 1e3) for d in per_level]
        return dict(levels=levels, mean=float(np.mean(levels)), sides=list(self.sides))
