"""Drop-in receiver API of the reference's `neuron_receivers` package.

Importing this package requires the sdmoe HIP library at call time (no CPU path). Hot-path receivers (MOEFy,
RemoveExperts, RemoveNeurons, WandaRemoveNeuronsFast, WandaRemovePerPrompt, MultiConceptRemoverWanda) plus the discovery
receivers that produce their inputs (GetExperts -> expert lists, Wanda -> column norms -> masks, NeuronPredictivity /
NeuronPredictivityBB -> max-activation statistics -> paired t-test or AP neuron masks; ExpertPredictivity -> per-expert
maximum routing scores -> paired t-test -> expert lists) and FrequencyMeasure, the per-expert
selection histogram for choosing topk_experts, and SparsityMeasure, the gate-sparsity counts of a relufied U-Net (the
measurement behind sparsity/check_sparsity.py's sparsity.json); the HPO path (BaseUNetReceiver, RemoveNeuronsHPO,
RemoveNeuronsNoiseHPO: the receivers modularity/remove_experts_hpo.py and remove_experts_noise_hpo.py drive, the noise
objective computed on the device by sdmoe_noise_distance), SaveStates, and AddExperts, the counterpart
of RemoveExperts: a per-expert score bias ahead of a top-k at int(0.8 k).
"""
from neuron_receivers.base_receiver import BaseNeuronReceiver, GEGLU, GELU  # noqa: F401
from neuron_receivers.predictivity import NeuronPredictivity  # noqa: F401
from neuron_receivers.neuron_predictivity_bb import NeuronPredictivityBB  # noqa: F401
from neuron_receivers.remove_skilled_neurons import RemoveNeurons  # noqa: F401
from neuron_receivers.moefy import MOEFy  # noqa: F401
from neuron_receivers.remove_skilled_experts import RemoveExperts  # noqa: F401
from neuron_receivers.add_skilled_experts import AddExperts  # noqa: F401
from neuron_receivers.remove_wanda_neurons_fast import WandaRemoveNeuronsFast  # noqa: F401
from neuron_receivers.remove_wanda_per_prompt import WandaRemovePerPrompt  # noqa: F401
from neuron_receivers.multi_concept_remover import MultiConceptRemoverWanda  # noqa: F401
from neuron_receivers.get_experts import GetExperts  # noqa: F401
from neuron_receivers.expert_activation import ExpertPredictivity  # noqa: F401
from neuron_receivers.frequency_measure import FrequencyMeasure  # noqa: F401
from neuron_receivers.sparsity_measure import SparsityMeasure  # noqa: F401
from neuron_receivers.wanda_receiver import Wanda  # noqa: F401
from neuron_receivers.base_unet_receiver import BaseUNetReceiver  # noqa: F401
from neuron_receivers.remove_skilled_neurons_hpo import RemoveNeuronsHPO  # noqa: F401
from neuron_receivers.remove_skilled_neurons_noise_hpo import RemoveNeuronsNoiseHPO  # noqa: F401
from neuron_receivers.save_states import SaveStates  # noqa: F401
