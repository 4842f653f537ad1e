"""GanClsEval — reference models/gancls/eval_gancls.py, which is models/wgancls/eval_wgan.py for a generator that returns the
image alone and takes no conditioning noise; the class count comes from EVAL.NUM_CLASSES.  The two modes are kept as the
reference has them: evaluate_inception runs the generator with is_training=False (eval_gancls.py:87: moving batch-norm
statistics — here the one-launch inference norm, kernels.bn_infer), evaluate_fid with the default is_training=True
(eval_gancls.py:41: batch statistics over each SAMPLE_SIZE batch; no moving average moves, there are no update ops in that graph).
evaluate_imd runs in eval mode.  All three are evaluation/evaluator.py's, stored."""
from ...evaluation.evaluator import GeneratorEval


class GanClsEval(GeneratorEval):
    def generate_batch(self, z, cond, is_training):
        return self.model.generator(z, cond, reuse=True, is_training=is_training)
