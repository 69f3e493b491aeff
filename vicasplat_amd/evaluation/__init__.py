from .evaluation_index_generator import EvaluationIndexGenerator, EvaluationIndexGeneratorCfg, IndexEntry, band_pairs  # noqa: F401
