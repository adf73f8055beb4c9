"""graphneuralnetwork_amd -- MI355X-native message-passing aggregation for the
GCN / GAT / GraphSAGE forward paths of kaddly/GraphNeuralNetwork.

Drop-in modules (same class names, constructor args, forward signatures and
state_dict keys as the reference):

* ``graphneuralnetwork_amd.gcn``       -- GCN_Model, Graph_conv_layer      (GCN/GCN.py)
* ``graphneuralnetwork_amd.gat``       -- GraphAttentionLayer, SpGraphAttentionLayer,
                                          GAT, SpGAT                       (GAT/models/*.py)
* ``graphneuralnetwork_amd.graphsage`` -- SageLayer, GraphSAGE, Aggregator (GraphSAGE/*.py)
* ``graphneuralnetwork_amd.loss``      -- supervised_loss, accuracy: the loss / accuracy /
                                          backward lines of the train_eval.py loops
* ``graphneuralnetwork_amd.gtn``       -- GTConv, GTLayer, GTN_Model, norm  (GTN/models/*.py);
                                          also importable from the package itself
* ``graphneuralnetwork_amd.gatne``     -- GraphEncoder, GraphDecoder, GATNEModel, SigmoidBCELoss,
                                          ValScale                     (GATNE_Pytorch/models/GATNE.py)

The aggregation hot paths run as hand-written gfx950 HIP kernels in
``lib/libgnn_mi355x.so`` behind the C-ABI of ``include/gnn_mi355x.h``.
"""
__version__ = "0.1.0"

_GTN = ("GTConv", "GTLayer", "GTN_Model")


def __getattr__(name):
    # resolved on first use: importing the package stays free of torch
    if name in _GTN:
        from . import gtn
        return getattr(gtn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
