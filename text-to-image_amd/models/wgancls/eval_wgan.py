"""WGanClsEval — the evaluator of the reference's models/wgancls/eval_wgan.py (what run.py starts when EVAL.FLAG is set;
here behind `run.py --eval is|fid`): evaluation/evaluator.py's stored evaluator over the wgancls generator, which returns
(image, mean, log sigma) and draws its conditioning noise.  IS runs it in eval mode (moving BN statistics), FID with
is_training=True, i.e. batch statistics over each SAMPLE_SIZE batch (the reference's default argument, kept)."""
from ...evaluation.evaluator import GeneratorEval


class WGanClsEval(GeneratorEval):
    def generate_batch(self, z, cond, is_training):
        return self.model.generator(z, cond, reuse=True, is_training=is_training)[0]
