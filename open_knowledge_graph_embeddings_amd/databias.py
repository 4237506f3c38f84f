"""The data-bias baselines: DataBiasOnly{Relation,Entity}Scorer and DataBiasOnly{Entity,Relation}Model
(openkge/model.py:281-350, :1036-1044) -- "how far do you get without the entity / without the relation".

Both models are the LSTM embedder (lstm.LSTMRelationEmbedder) under a scorer whose query row is ONE encoded row, copied:

    scorer                        sp rows          po rows
    DataBiasOnlyRelationScorer    rel . obj^T      rel . subj^T       ("bias_relation", OKGE_BIAS_RELATION)
    DataBiasOnlyEntityScorer      subj . obj^T     obj . subj^T       ("bias_entity",   OKGE_BIAS_ENTITY)

The other prefix slot is still encoded (model.py:58-59, :72-73) but never reaches the score.  So in the entity model no relation
parameter has a gradient -- torch optimizers skip them, they stay bit-unchanged -- while the relation batch-norm's running
statistics still move; in the relation model the entities learn through the candidate rows only.  Nothing here is a new model
stack: the scorers are two scorer kinds of the C ABI (the fold is a copy inside the existing kernels, the chain rule is
csrc/okge_bias.hip), the step is lstm.LSTMTrainStep, which leaves the unused relation slot untouched.

Triple scoring raises, as in the reference (model.py:311-312, :347-348).
"""
from __future__ import annotations

from .lstm import LSTMRelationEmbedder
from .model import Models, RelationScorer


def _prefix_only_score(self, subj, rel, obj, prefix, sp, po):
    """prefix scoring only: RelationScorer's HIP paths (okge_score_prefixes; PrefixScoreFn with gradients enabled) under the
    class's scorer kind; anything else raises as the reference does (model.py:311-312, :347-348)"""
    if not prefix:
        raise Exception
    return RelationScorer._score(self, subj, rel, obj, prefix=True, sp=sp, po=po)


class DataBiasOnlyRelationScorer(RelationScorer):
    """openkge/model.py:281-314"""
    scorer_name = "bias_relation"

    def triple_score(self, subj, rel, obj, drop_relation=False):
        return self._score(subj, rel, obj)

    def _score(self, subj, rel, obj, prefix=False, drop_relation=False, sp=None, po=None):
        return _prefix_only_score(self, subj, rel, obj, prefix, sp, po)


class DataBiasOnlyEntityScorer(RelationScorer):
    """openkge/model.py:317-350"""
    scorer_name = "bias_entity"

    def triple_score(self, subj, rel, obj, drop_relation=False):
        return self._score(subj, rel, obj)

    def _score(self, subj, rel, obj, prefix=False, drop_relation=False, sp=None, po=None):
        return _prefix_only_score(self, subj, rel, obj, prefix, sp, po)


class DataBiasOnlyEntityModel(DataBiasOnlyEntityScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)

    def autograd_params_and_grads(self, st):
        """AddLossModule bridge: the relation parameters are left out, so their `.grad` stays None and a torch optimizer
        skips them, as after the reference's backward"""
        params, grads = [self.entity_embedding.weight], [st.entity.dW]
        bn = self.entity_batchnorm
        if bn is not None:
            params += [bn.weight, bn.bias]
            grads += [st.entity.d_bn[:st.entity.d], st.entity.d_bn[st.entity.d:]]
        params += self._lstm_tensors(self.entity_encoder_in)
        grads += st.entity.dlstm
        return params, grads


class DataBiasOnlyRelationModel(DataBiasOnlyRelationScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.DataBiasOnlyEntityModel = DataBiasOnlyEntityModel
Models.DataBiasOnlyRelationModel = DataBiasOnlyRelationModel
