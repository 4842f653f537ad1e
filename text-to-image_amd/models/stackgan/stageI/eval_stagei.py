"""StageIEval — reference models/stackgan/stageI/eval_stagei.py, which is models/wgancls/eval_wgan.py with the class count taken
from EVAL.NUM_CLASSES: evaluation/evaluator.py's stored evaluator (the Stage-I generator lives under `g_net` with the wgancls
generator's signature).  IS and IMD with the generator in eval mode, FID with is_training=True."""
from ....evaluation.evaluator import GeneratorEval


class StageIEval(GeneratorEval):
    def generate_batch(self, z, cond, is_training):
        return self.model.generator(z, cond, reuse=True, is_training=is_training)[0]
