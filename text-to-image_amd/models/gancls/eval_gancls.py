"""GanClsEval — reference models/gancls/eval_gancls.py, which is models/wgancls/eval_wgan.py for a generator that returns the
image alone and takes no conditioning noise; the class count comes from EVAL.NUM_CLASSES.  The two modes are kept as the
reference has them: evaluate_inception runs the generator with is_training=False (eval_gancls.py:87: moving batch-norm
statistics — here the one-launch inference norm, kernels.bn_infer), evaluate_fid with the default is_training=True
(eval_gancls.py:41: batch statistics over each SAMPLE_SIZE batch; no moving average moves, there are no update ops in that graph).

evaluate_imd is StageIEval's addition (evaluation/imd.py): each real test image against the image generated from its embedding,
eval-mode batch norm."""
import torch

from ..stackgan.stageI.eval_stagei import StageIEval


class GanClsEval(StageIEval):
    def _generate_batch(self, z, cond, is_training):
        return self.model.generator(z, cond, reuse=True, is_training=is_training)

    def _generate(self, is_training):
        """-> device float32 [SIZE // bs * bs, H, W, 3]: WGanClsEval._generate's draws (z ~ N(0, 1), then the test batch) through this
        model's generator."""
        m = self.model
        n_batches = self._n_batches()
        h, w, c = m.image_dims[0], m.image_dims[1], m.image_dims[2]
        samples = torch.empty((n_batches * self.bs, h, w, c), dtype=torch.float32, device=m.device)
        for i in range(n_batches):
            print('\rGenerating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
            _, z, cond = self._draw_batch(*self._dims())
            with torch.no_grad():
                img = self._generate_batch(z, cond, is_training)
            samples[i * self.bs:(i + 1) * self.bs].copy_(img.float().reshape(self.bs, h, w, c))
        print()
        return samples
