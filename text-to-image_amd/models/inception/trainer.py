"""InceptionTrainer — reference models/inception/trainer.py: fine-tunes InceptionV3 on the dataset's TEST split (classes the GANs
never see) so that the Inception score and FID of the GANs are measured by a network that knows those classes.

Semantics kept from the reference: labels mapped through `test.class_to_index()`; `RESTORE_PRETRAIN` restores every variable but
Logits/* and AuxLogits/* from PRETRAINED_CHECKPOINT_DIR and starts at step 0 (logits weights ~ truncated_normal(0.1), biases 0,
RMSProp slots `rms` = 1 and `momentum` = 0), otherwise the run resumes from CHECKPOINT_DIR and a failed load raises; the loop runs
`for idx in range(start + 1, MAX_STEPS)`; every SUMMARY_PERIOD steps a summary (`loss`, `image`, `train_acc`) computed by a SECOND
training-mode forward after the update (fresh dropout, no moving-average update) and the line
`Epoch: [%2d] [%4d] time: %4.4f, loss: %.8f` with the step's own loss; a checkpoint every 200 steps, CHECKPOINTS_TO_KEEP kept.
PRETRAINED_CHECKPOINT_DIR names an npz keyed by slim's variable names (train_net.pretrained_arrays)."""
import sys
import time

import numpy as np
import torch

from ... import kernels as K
from ...utils import summary as S
from ...utils.saver import Saver, load, save
from .model import variable_shapes
from .train_net import LOGITS, InceptionTrainNet, pretrained_arrays

SAVE_PERIOD = 200


class InceptionTrainer(object):
    def __init__(self, sess, dataset, cfg, device=None):
        self.sess = sess                    # (no TF session; kept for the reference's signature)
        self.dataset = dataset
        self.class_to_idx = self.dataset.test.class_to_index()
        self.cfg = cfg
        self.device = device or torch.device('cuda', torch.cuda.current_device())
        self.net = None

    def define_model(self):
        """The network's variables: restored from the pretrained npz (+ freshly initialised logits) or, for a resume, placeholders
        that the checkpoint load overwrites."""
        C = self.cfg.MODEL.CLASSES
        shapes = variable_shapes(C)
        if self.cfg.TRAIN.RESTORE_PRETRAIN:
            arrays = pretrained_arrays(self.cfg.TRAIN.PRETRAINED_CHECKPOINT_DIR, C)
        else:
            arrays = {}
        for key, shape in shapes.items():
            if key not in arrays:
                arrays[key] = np.zeros(shape, np.float32)
        self.net = InceptionTrainNet(arrays, C, self.device, seed=int(self.cfg.TRAIN.get('SEED', 0)))
        if self.cfg.TRAIN.RESTORE_PRETRAIN:
            with torch.no_grad():
                K.trunc_normal_(self.net.weights[LOGITS], 0.0, 0.1)        # slim's arg-scope initializer; biases stay 0
            K.filter_cache_invalidate()

    def train(self):
        cfg = self.cfg
        self.define_model()
        self.writer = S.FileWriter(cfg.LOGS_DIR)
        start_time = time.time()
        self.saver = Saver(self.net.store, optimizers={'': self.net.opt}, max_to_keep=cfg.TRAIN.CHECKPOINTS_TO_KEEP)
        if cfg.TRAIN.RESTORE_PRETRAIN:
            start_point = 0
        else:
            could_load, checkpoint_counter = load(self.saver, None, cfg.CHECKPOINT_DIR)
            if could_load:
                start_point = checkpoint_counter
                print(' [*] Load SUCCESS')
            else:
                print(' [!] Load failed...')
                raise RuntimeError('Failed to restore the complete Inception model')
        sys.stdout.flush()

        batch_size = cfg.TRAIN.BATCH_SIZE
        C = cfg.MODEL.CLASSES
        last = None
        for idx in range(start_point + 1, cfg.TRAIN.MAX_STEPS):
            epoch_size = self.dataset.test.num_examples // batch_size
            epoch = idx // epoch_size

            images, _, _, _, labels = self.dataset.test.next_batch(batch_size, labels=True)
            new_labels = np.array([self.class_to_idx[label] for label in labels], np.int32)
            assert np.min(new_labels) >= 0 and np.max(new_labels) < C
            lab = torch.from_numpy(new_labels).to(self.device)

            head = self.net.step(images, lab, 2 * idx)
            err = float(head['loss'].item())

            if np.mod(idx, cfg.TRAIN.SUMMARY_PERIOD) == 0:
                ev = self.net.evaluate(images, lab, 2 * idx + 1)
                self.writer.add_summary([S.scalar('loss', float(ev['loss'].item())), S.image('image', images.cpu().numpy()),
                                         S.scalar('train_acc', float(ev['acc'].item()))], idx)
                self.writer.flush()
                print('Epoch: [%2d] [%4d] time: %4.4f, loss: %.8f' % (epoch, idx, time.time() - start_time, err))

            if np.mod(idx, SAVE_PERIOD) == 0:
                save(self.saver, None, cfg.CHECKPOINT_DIR, idx)
            last = dict(step=idx, loss=err, acc=float(head['acc'].item()))
            sys.stdout.flush()
        self.writer.close()
        return last
