"""Checkpoints — the role of the reference's utils/saver.py:6-25 (tf.train.Saver save / restore by global step).

On-disk format: one `<prefix>-<step>.npz` per checkpoint holding every variable of the store under its TF name
(`d_net/Conv_3/weights`, `g_net/BatchNorm_4/moving_mean`, ... — conv kernels HWIO, deconv [kh,kw,Cout,Cin], dense
[in,out], i.e. exactly the key space and layouts of the reference's TF checkpoints, so arrays dumped from a real TF run
load unchanged), plus optimizer slots under `<opt>/<name>/Adam` and `/Adam_1` and the step counts `<opt>/t` (an optimizer with `slots()` names its own
slots through `slot_key`: optim.RMSPropTF writes TF's `<name>/RMSProp` and `/RMSProp_1`) and whatever
scalars the trainer registers through `extra` (wgancls: `kt` and `global_step`); with `shadows`, the exponential moving average of every saved arena
variable under TF's own shadow name `<name>/ExponentialMovingAverage`; and a `checkpoint` text file naming the latest one (what tf.train.get_checkpoint_state reads).  `load`
returns (found, counter) with the counter parsed from the file name like the reference does."""
import os
import re

import numpy as np
import torch


class Saver(object):
    """var_list: name prefixes to include (None = every variable), like tf.train.Saver(var_list).
    shadows: optimizers that carry an `ema` over their arena (optim.AdamTF(ema_decay=...)).  Every arena variable that var_list
    selects is also written under `<variable>/ExponentialMovingAverage`; restore() reads that key where the file has it and
    otherwise sets the slot from the variable it has just restored (a checkpoint written without EMA, a variable new at this
    stage); arena variables outside var_list keep the shadow they have.  shadows=None: the files are what they were without it."""

    def __init__(self, store, optimizers=None, extra=None, var_list=None, max_to_keep=5, shadows=None):
        self.store, self.optimizers, self.extra = store, optimizers or {}, extra or {}
        self.var_list, self.max_to_keep = var_list, max_to_keep
        self.shadows = list(shadows.values() if isinstance(shadows, dict) else shadows) if shadows else []
        for opt in self.shadows:
            if getattr(opt, 'ema', None) is None:
                raise ValueError('shadows: %r keeps no moving average (ema_decay=None)' % (opt,))
        self._kept = []

    def _is_selected(self, n):
        return self.var_list is None or any(n.startswith(p) for p in self.var_list)

    def _selected(self):
        for n, v in self.store.vars.items():
            if self._is_selected(n):
                yield n, v

    def _shadow_slots(self):
        """(key, shadow slot, weight slot) of every selected arena variable of every shadow-carrying optimizer."""
        for opt in self.shadows:
            a = opt.arena
            for n in a.names:
                if n in self.store.vars and self._is_selected(n):
                    o, k = a.offsets[n]
                    yield shadow_key(n), opt.ema[o:o + k].view(a.vars[n].shape), a.flat[o:o + k].view(a.vars[n].shape)

    def state(self):
        out = {n: v.detach().cpu().numpy() for n, v in self._selected()}
        for key, shadow, _ in self._shadow_slots():
            out[key] = shadow.detach().cpu().numpy()
        for oname, opt in self.optimizers.items():
            a = opt.arena
            if hasattr(opt, 'slots'):            # an optimizer that names its own slots (optim.RMSPropTF)
                for n in a.names:
                    o, k = a.offsets[n]
                    for slot, buf in opt.slots().items():
                        out[opt.slot_key(oname, n, slot)] = buf[o:o + k].view(a.vars[n].shape).cpu().numpy()
                continue
            for n in a.names:
                o, k = a.offsets[n]
                out['%s/%s/Adam' % (oname, n)] = opt.m[o:o + k].view(a.vars[n].shape).cpu().numpy()
                out['%s/%s/Adam_1' % (oname, n)] = opt.v[o:o + k].view(a.vars[n].shape).cpu().numpy()
            out['%s/t' % oname] = np.array(opt.t)
        for k, get in self.extra.items():
            out[k] = np.asarray(get[0]())
        return out

    def restore(self, path, ema=False):
        """ema=True: every selected variable is loaded from its shadow key instead of its own (the averaged weights as the
        weights: evaluation and visualisation); a file without that key was trained without EMA — KeyError."""
        z = np.load(path)
        with torch.no_grad():
            for n, v in self._selected():
                key = shadow_key(n) if ema and getattr(self.store, 'trainable', {}).get(n, True) else n      # (a variable no optimizer steps has no shadow: PGGAN's w_avg)
                if key not in z.files:
                    if ema:
                        raise KeyError('checkpoint %s has no %s: it was trained without EMA (no moving average of the weights was kept)'
                                       % (path, key))
                    raise KeyError('checkpoint %s has no variable %s' % (path, n))
                if tuple(z[key].shape) != tuple(v.shape):
                    raise ValueError('checkpoint %s: %s has shape %s, variable has %s' % (path, key, z[key].shape, tuple(v.shape)))
                v.copy_(torch.from_numpy(z[key]).to(v.device))
            for key, shadow, weight in self._shadow_slots():
                if key in z.files:
                    if tuple(z[key].shape) != tuple(shadow.shape):
                        raise ValueError('checkpoint %s: %s has shape %s, variable has %s' % (path, key, z[key].shape, tuple(shadow.shape)))
                    shadow.copy_(torch.from_numpy(z[key]).to(shadow.device))
                else:
                    shadow.copy_(weight)
            for oname, opt in self.optimizers.items():
                a = opt.arena
                if hasattr(opt, 'slots'):
                    for n in a.names:
                        o, k = a.offsets[n]
                        for slot, buf in opt.slots().items():
                            key = opt.slot_key(oname, n, slot)
                            if key not in z.files:
                                raise KeyError('checkpoint %s has no optimizer slot %s' % (path, key))
                            buf[o:o + k].copy_(torch.from_numpy(z[key]).reshape(-1).to(buf.device))
                    continue
                for n in a.names:
                    o, k = a.offsets[n]
                    if '%s/%s/Adam' % (oname, n) in z.files:
                        opt.m[o:o + k].copy_(torch.from_numpy(z['%s/%s/Adam' % (oname, n)]).reshape(-1).to(opt.m.device))
                        opt.v[o:o + k].copy_(torch.from_numpy(z['%s/%s/Adam_1' % (oname, n)]).reshape(-1).to(opt.v.device))
                if '%s/t' % oname in z.files:
                    opt.t = int(z['%s/t' % oname])
                if hasattr(opt, 'moments_loaded'):
                    opt.moments_loaded()
            for k, get in self.extra.items():
                if k in z.files:
                    get[1](z[k])
        from .. import kernels as K
        K.filter_cache_invalidate()


def shadow_key(name):
    """tf.train.ExponentialMovingAverage names the shadow of a variable `<variable>/ExponentialMovingAverage`."""
    return '%s/ExponentialMovingAverage' % name


_CKPT_RE = re.compile(r'^model-(\d+)\.npz$')


def _existing(checkpoint_dir):
    """Checkpoints already in the directory, oldest step first (what max_to_keep prunes against after a resume)."""
    found = []
    if os.path.isdir(checkpoint_dir):
        for f in os.listdir(checkpoint_dir):
            m = _CKPT_RE.match(f)
            if m:
                found.append((int(m.group(1)), os.path.join(checkpoint_dir, f)))
    return [p for _, p in sorted(found)]


def save(saver, sess, checkpoint_dir, step):
    """reference utils/saver.py:6-10 (sess is unused: there is no TF session).  The archive is written to a temporary
    name and renamed into place, so a crash mid-save never leaves a truncated newest checkpoint; the `checkpoint` state
    file is updated only after the archive exists."""
    if not os.path.exists(checkpoint_dir):
        os.makedirs(checkpoint_dir)
    name = 'model-%d.npz' % step
    path = os.path.join(checkpoint_dir, name)
    tmp = path + '.tmp'
    with open(tmp, 'wb') as f:
        np.savez(f, **saver.state())
    os.replace(tmp, path)
    saver._kept = [p for p in _existing(checkpoint_dir) if p != path] + [path]
    while len(saver._kept) > saver.max_to_keep:
        old = saver._kept.pop(0)
        if os.path.exists(old):
            os.remove(old)
    state_tmp = os.path.join(checkpoint_dir, 'checkpoint.tmp')
    with open(state_tmp, 'w') as f:
        f.write('model_checkpoint_path: "%s"\n' % name)
    os.replace(state_tmp, os.path.join(checkpoint_dir, 'checkpoint'))
    return path


def latest_checkpoint(checkpoint_dir):
    """The archive `load` reads: the one the directory's `checkpoint` state file names, if both exist (a newer archive the state file
    does not name is not it); else None."""
    state = os.path.join(checkpoint_dir, 'checkpoint')
    if os.path.isfile(state):
        m = re.search(r'model_checkpoint_path: "([^"]+)"', open(state).read())
        if m and os.path.isfile(os.path.join(checkpoint_dir, m.group(1))):
            return os.path.join(checkpoint_dir, os.path.basename(m.group(1)))
    return None


def load(saver, sess, checkpoint_dir, ema=False):
    """reference utils/saver.py:13-25 -> (could_load, counter).  ema: Saver.restore's."""
    print(' [*] Reading checkpoints from %s...' % checkpoint_dir)
    path = latest_checkpoint(checkpoint_dir)
    if path is None:
        print(' [*] Failed to find checkpoints')
        return False, 0
    ckpt_name = os.path.basename(path)
    saver.restore(path, ema=ema)
    saver._kept = _existing(checkpoint_dir)          # pruning continues across the resume
    counter = int(next(re.finditer(r'(\d+)(?!.*\d)', ckpt_name)).group(0))
    print(' [*] Success to read {}'.format(ckpt_name))
    return True, counter


def restore_scopes(store, pairs, create=None, error=RuntimeError, verbose=True, ema=False, extra=None):
    """Restores each (scope, directory) of `pairs` in order: tf.train.Saver(tf.global_variables(scope)) + load in the reference.
    When the last scope has no trainable variables yet, `create()` builds the generators once, launch-free (K.dry_run, no gradient).
    The first directory without a checkpoint ends it: ` [!] Load failed...` and `raise error(scope)` (the caller's exception); a
    restored one prints ` [*] Load SUCCESS`.  verbose=False drops those two lines (load's own remain).  ema=True loads every variable
    from its `<variable>/ExponentialMovingAverage` key (KeyError for a checkpoint trained without EMA).  extra: Saver's `extra`
    ({key: (getter, setter)}), handed to every scope's Saver: a setter is called with the entry of each checkpoint that has its key
    (default None: no entry is read)."""
    if create is not None and not store.trainable_variables(pairs[-1][0]):
        from .. import kernels as K
        with K.dry_run(), torch.no_grad():
            create()
    for scope, directory in pairs:
        could_load, _ = load(Saver(store, var_list=[scope], extra=extra), None, directory, ema=ema)
        if not could_load:
            if verbose:
                print(' [!] Load failed...')
            raise error(scope)
        if verbose:
            print(' [*] Load SUCCESS')


def restore_g_net(model, directory, batch, error, ema=False):
    """`g_net` of a model whose generator takes (z [batch, z_dim], embedding [batch, embed_dim]), from `directory`."""
    def create():
        model.generator(torch.empty(batch, model.z_dim, device=model.device), torch.empty(batch, model.embed_dim, device=model.device),
                        reuse=False, is_training=False)
    restore_scopes(model.store, [('g_net', directory)], create, lambda scope: error, ema=ema)
