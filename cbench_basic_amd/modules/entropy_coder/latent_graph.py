"""Latent-graph entropy model driver -- API of LatentGraphicalANSEntropyCoder
(cbench/modules/entropy_coder/latent_graph.py:306) restricted to the encode / decode /
update_state hot path:

    encode:  node generators -> inference edges (x->y->z: g_a, h_a) -> generative pass
             (z then y): per node  forward (quantise)  +  encode (bytes),  generative edges
             (z->y: h_s)                                     latent_graph.py:1232-1264, :721, :760
    decode:  split bytes -> generative pass z -> y -> x (h_s, g_s)      latent_graph.py:1266-1295
    stream:  merge_bytes([bytes_z, bytes_y], num_segments=2)            utils/bytes_ops.py:19-33

Graph traversal is tiny host logic; every tensor operation it triggers is a HIP kernel.
Training-only machinery (losses, MC sampling, FLOPs regularisers, sandwich rule) is out of
scope.  The greedy complexity-level search of BaSIC (post_training_process, latent_graph.py:1397-1640) is here:
selection logic in complexity_search.py, evaluation = this codec's own forward on the GPU; a ready-made result
(per-level node parameters) can also be installed with ``set_complexity_level_params``.
"""
from typing import Any, Dict, Iterable, List, Optional

import math
import struct
import time
import numpy as np
import torch
import torch.nn as nn

from ...base import HotPathModule
from ...codecs.base import (VariableComplexityCodecInterface, VariableRateCodecInterface,
                            VariableTaskCodecInterface)
from ...utils.bytes_ops import merge_bodies, merge_bytes, split_merged_bytes, split_merged_views
from ...utils import item_framing
from ...utils.qstep import check_qsteps
from .complexity_search import search_complexity_levels


class LossyDummyEntropyCoder(HotPathModule):
    """latent_graph.py:68-144: the input node of a lossy codec carries no bits; decoding
    returns the prior (= g_s output)."""

    def __init__(self, *args, lambda_rd=1.0, distortion_type="mse", **kwargs):
        super().__init__()
        self.lambda_rd = lambda_rd
        self.distortion_type = distortion_type

    def forward(self, data, *args, prior=None, lambda_rd=None, prior_target=None, **kwargs):
        """latent_graph.py:121-141: distortion metrics of the reconstruction (= prior).  metric_dict gets ``mse`` and
        ``weighted_distortion`` = lambda_rd * (sum of squared errors per image, averaged over the batch) (:83-88,:139)."""
        if isinstance(data, torch.Tensor) and isinstance(prior, torch.Tensor):
            if self.distortion_type not in ("mse", "ms-ssim"):
                raise NotImplementedError(f"distortion_type {self.distortion_type}")
            target = data if prior_target is None else prior_target
            rec = prior
            for dim, size in enumerate(target.shape[2:], 2):  # crop to the target size (:127-129)
                if rec.shape[dim] != size:
                    rec = rec.narrow(dim, 0, size)
            if self.distortion_type == "ms-ssim":
                # :92-96 (the "...-ft-ssim" presets): loss = mean over the batch of (1 - MS-SSIM) x elements per image; the metric
                # comes from benchmark/ms_ssim.py, a restatement of the absent pytorch_msssim package (parity-unpinned)
                from ...benchmark.ms_ssim import ms_ssim
                val = ms_ssim(rec, target, data_range=1.0, size_average=False)
                loss_distortion = (1 - val).mean() * (target.numel() // target.shape[0])
                self.update_cache("metric_dict", ms_ssim=val.mean(),
                                  weighted_distortion=loss_distortion * (self.lambda_rd if lambda_rd is None else lambda_rd))
                return rec
            from ...nn import kernels as K
            mse = K.mse_per_image(rec.contiguous(), target.contiguous())  # [B], HIP reduction
            loss_distortion = (mse * (target.numel() // target.shape[0])).mean()
            self.update_cache("metric_dict", mse=mse.mean(),
                              weighted_distortion=loss_distortion * (self.lambda_rd if lambda_rd is None else lambda_rd))
            return rec     # the reference returns the NARROWED prior (:121-123,:141): forward() is input-sized, decode() is not
        return prior

    def encode(self, data, *args, prior=None, **kwargs) -> bytes:
        return b""

    def decode(self, byte_string: bytes, *args, prior=None, **kwargs):
        return prior

    def update_state(self, *args, **kwargs):
        pass

    # item framing (utils/item_framing.py): a node without bits has an empty body at any batch size
    can_split_items = True

    def split_items(self, body, n, **ctx):
        return item_framing.empty_split(body, n)

    def merge_items(self, bodies, **ctx):
        return item_framing.empty_merge(bodies)

    def item_shape(self, body, **ctx):
        return None


class ParamDictModuleWrapper(nn.Module):
    """latent_graph.py:270-298: keeps a dict of node values as buffers so the searched complexity levels travel in the
    state_dict under the reference's keys (``_complexity_param_all_levels.<level>.<node>``)."""

    def __init__(self, params: Dict[str, Any]):
        super().__init__()
        self.none_params = []
        for name, value in params.items():
            if value is None:
                self.none_params.append(name)
            elif isinstance(value, dict):
                setattr(self, name, ParamDictModuleWrapper(value))
            else:
                self.register_buffer(name, torch.as_tensor(value).detach().clone())

    def forward(self, *args, **kwargs):
        out = {name: None for name in self.none_params}
        out.update(self._buffers)
        for name, m in self._modules.items():
            out[name] = m()
        return out


class BasicLatentGraphicalNodeAggregatorModel(nn.Module):
    """latent_graph.py:55-60: folds the list of values several edges delivered to one node."""

    def forward(self, input_list, *args, **kwargs):
        raise NotImplementedError()


class AverageNodeAggregatorModel(BasicLatentGraphicalNodeAggregatorModel):
    """latent_graph.py:63-65."""

    def forward(self, input_list, *args, **kwargs):
        return torch.stack(input_list).mean(0)


class LatentGraphicalANSEntropyCoder(HotPathModule, VariableRateCodecInterface, VariableComplexityCodecInterface,
                                     VariableTaskCodecInterface):
    DEFAULT_EDGE_SPLIT_SYMBOL = "_"
    DEFAULT_PRIOR_KEY_NAME = "prior"
    DEFAULT_UNCONDITIONAL_NODE_NAME = "u"
    DEFAULT_INPUT_NODE_NAME = "x"
    DEFAULT_RATE_LEVEL_NODE_NAME = "vrlevel"
    DEFAULT_COMPLEX_LEVEL_NODE_NAME = "sclevel"
    DEFAULT_TASK_INDEX_NODE_NAME = "taskidx"

    def __init__(self, *args,
                 use_lossy_compression=True,
                 lossy_compression_lambda_rd=1.0,
                 lossy_compression_distortion_type="mse",
                 node_generator_dict: Dict[str, nn.Module] = None,
                 node_generator_input_mapping: Optional[Dict[str, Dict[str, str]]] = None,
                 dynamic_node_generator_dict: Dict[str, nn.Module] = None,
                 latent_node_entropy_coder_dict: Dict[str, nn.Module] = None,
                 latent_inference_dict: Dict[str, nn.Module] = None,
                 latent_generative_dict: Dict[str, nn.Module] = None,
                 latent_inference_input_mapping: Optional[Dict[str, Dict[str, str]]] = None,
                 latent_generative_input_mapping: Optional[Dict[str, Dict[str, str]]] = None,
                 latent_node_inference_topo_order: Optional[List[str]] = None,
                 latent_node_generative_topo_order: Optional[List[str]] = None,
                 latent_inference_node_aggregator_dict: Optional[Dict[str, nn.Module]] = None,
                 latent_generative_node_aggregator_dict: Optional[Dict[str, nn.Module]] = None,
                 complexity_metric_list=None,
                 complexity_level_greedy_search=False,
                 complexity_level_greedy_search_dataset: Optional[Iterable] = None,
                 complexity_level_greedy_search_dataset_cached=False,
                 complexity_level_greedy_search_iterative=False,
                 complexity_level_greedy_search_num_levels: Optional[int] = None,
                 complexity_level_greedy_search_custom_constraint: Optional[List[float]] = None,
                 complexity_level_greedy_search_performance_metric: Optional[str] = None,
                 complexity_level_greedy_search_complexity_metric: Optional[str] = None,
                 complexity_level_greedy_search_add_controller_nodes_as_complexity_metric=True,
                 complexity_level_controller_nodes=(),
                 complexity_level_greedy_search_custom_params: Optional[List[Dict[str, int]]] = None,
                 complexity_level_greedy_search_loss_mode="eval",
                 task_names: Optional[List[str]] = None,
                 **kwargs):
        super().__init__()
        node_generator_dict = dict(node_generator_dict or {})
        dynamic_node_generator_dict = dict(dynamic_node_generator_dict or {})
        latent_node_entropy_coder_dict = dict(latent_node_entropy_coder_dict or {})
        self.use_lossy_compression = use_lossy_compression
        if use_lossy_compression and self.DEFAULT_INPUT_NODE_NAME not in latent_node_entropy_coder_dict:
            latent_node_entropy_coder_dict[self.DEFAULT_INPUT_NODE_NAME] = LossyDummyEntropyCoder(
                lambda_rd=lossy_compression_lambda_rd, distortion_type=lossy_compression_distortion_type)

        self.node_generators = nn.ModuleDict(node_generator_dict)
        self.node_generator_input_mapping = dict(node_generator_input_mapping or {})
        self.dynamic_node_generators = nn.ModuleDict(dynamic_node_generator_dict)
        self.latent_node_entropy_coders = nn.ModuleDict(latent_node_entropy_coder_dict)
        self.latent_inference_modules = nn.ModuleDict(dict(latent_inference_dict or {}))
        self.latent_generative_modules = nn.ModuleDict(dict(latent_generative_dict or {}))
        self.latent_inference_input_mapping = dict(latent_inference_input_mapping or {})
        self.latent_generative_input_mapping = dict(latent_generative_input_mapping or {})
        # multi-edge aggregators (latent_graph.py:343-344,467-468): a node fed by SEVERAL edges collects their outputs in a list,
        # the node's aggregator folds it.  Same attribute names as the reference: they are state_dict prefixes
        self.latent_inference_node_aggregator_modules = nn.ModuleDict(dict(latent_inference_node_aggregator_dict or {}))
        self.latent_generative_node_aggregator_modules = nn.ModuleDict(dict(latent_generative_node_aggregator_dict or {}))
        self.latent_node_inference_topo_order = list(latent_node_inference_topo_order)
        self.latent_node_generative_topo_order = list(latent_node_generative_topo_order)
        self.complexity_level_greedy_search = complexity_level_greedy_search
        self.complexity_level_controller_nodes = list(complexity_level_controller_nodes)
        self.task_names = task_names

        # edges grouped by destination / source node (latent_graph.py:546-558)
        sym = self.DEFAULT_EDGE_SPLIT_SYMBOL
        self._inference_edges_into = {n: [] for n in self.latent_node_inference_topo_order}
        for edge in self.latent_inference_modules:
            self._inference_edges_into[edge.split(sym)[1]].append(edge)
        self._generative_edges_from = {n: [] for n in self.latent_node_generative_topo_order}
        for edge in self.latent_generative_modules:
            self._generative_edges_from[edge.split(sym)[0]].append(edge)

        # variable rate / complexity / task bookkeeping (latent_graph.py:566-648)
        def _levels(name):
            if name in self.dynamic_node_generators:
                g = self.dynamic_node_generators[name]
                return g.max_sample - g.min_sample + 1
            return 0
        self._num_rate_levels = _levels(self.DEFAULT_RATE_LEVEL_NODE_NAME)
        self._num_tasks = _levels(self.DEFAULT_TASK_INDEX_NODE_NAME)
        self._num_complex_levels = _levels(self.DEFAULT_COMPLEX_LEVEL_NODE_NAME)
        self._current_rate_level = -1
        self._current_task_idx = -1
        self._current_complex_level = -1
        self._complexity_param_all_levels = None  # ModuleList of ParamDictModuleWrapper, one per level
        self._searching = False  # True while post_training_process evaluates explicit controller settings
        self._valid_host = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_valid_host", None))
        # greedy complexity-level search (latent_graph.py:590-634)
        self.complexity_metric_list = list(complexity_metric_list or [])
        self.complexity_level_greedy_search_dataset = complexity_level_greedy_search_dataset
        self.complexity_level_greedy_search_dataset_cached = complexity_level_greedy_search_dataset_cached
        self.complexity_level_greedy_search_iterative = complexity_level_greedy_search_iterative
        self.complexity_level_greedy_search_custom_constraint = complexity_level_greedy_search_custom_constraint
        self.complexity_level_greedy_search_custom_params = complexity_level_greedy_search_custom_params
        # "eval": the loss on the rounded latents the codec codes (deterministic, the default here); "train": the reference's
        # own evaluation (latent_graph.py:1322 self.train()): additive-uniform-noise proxies in every coder, a random variable
        if complexity_level_greedy_search_loss_mode not in ("eval", "train"):
            raise ValueError("complexity_level_greedy_search_loss_mode: 'eval' or 'train'")
        self.complexity_level_greedy_search_loss_mode = complexity_level_greedy_search_loss_mode
        self.complexity_level_greedy_search_complexity_metric = complexity_level_greedy_search_complexity_metric
        self.complexity_level_greedy_search_performance_metric = complexity_level_greedy_search_performance_metric
        if complexity_level_greedy_search:
            if complexity_level_greedy_search_num_levels is not None:
                self._num_complex_levels = complexity_level_greedy_search_num_levels
            elif complexity_level_greedy_search_custom_constraint is not None:
                self._num_complex_levels = len(complexity_level_greedy_search_custom_constraint)
            valid = False
            if complexity_level_greedy_search_custom_params is not None:
                levels = [{k: self.node_generators[k](v) for k, v in idx.items()}
                          for idx in complexity_level_greedy_search_custom_params]
                self._num_complex_levels = len(levels)
            else:  # every level starts as the most complex setting until post_training_process has run (:604-615)
                most = {k: self.node_generators[k](self.node_generators[k].min_sample) for k in self.complexity_level_controller_nodes}
                levels = [most for _ in range(self._num_complex_levels)]
            self._complexity_param_all_levels = nn.ModuleList([ParamDictModuleWrapper(lv) for lv in levels])
            self.register_buffer("_complexity_param_valid", torch.tensor([valid]))
            if self.complexity_level_greedy_search_complexity_metric is None:
                self.complexity_level_greedy_search_complexity_metric = "FLOPs"
            self.complexity_metric_list.append(self.complexity_level_greedy_search_complexity_metric)
            if self.complexity_level_greedy_search_performance_metric is None:
                self.complexity_level_greedy_search_performance_metric = "loss"
            self.complexity_metric_list.append(self.complexity_level_greedy_search_performance_metric)
            if complexity_level_greedy_search_add_controller_nodes_as_complexity_metric:
                self.complexity_metric_list.extend(self.complexity_level_controller_nodes)
        if self._num_complex_levels > 0 and len(self.complexity_metric_list) > 0:  # (:641-645)
            self.register_buffer("_complexity_metric_list_cache",
                                 torch.zeros(self._num_complex_levels, len(self.complexity_metric_list)))
        if self._num_tasks > 0 and self.task_names is None:
            self.task_names = list(range(self._num_tasks))

    # Optional callable run by encode() right after the analysis transforms have been ENQUEUED on the current HIP stream
    # (before the entropy stage): concurrent stream workers use it to order their transform phases (benchmark/stream_workers.py).
    after_inference_hook = None

    def _levels_valid(self):
        """_complexity_param_valid as a host bool (read once; refreshed after load_state_dict / search)."""
        if self._valid_host is None:
            self._valid_host = bool(self._complexity_param_valid.item())
        return self._valid_host

    # ---- default nodes (latent_graph.py:650-683)
    def _get_default_node_dict(self, force_add_default_dynamic_nodes=False, **kwargs):
        out = {self.DEFAULT_UNCONDITIONAL_NODE_NAME: None, **kwargs}
        if self.training:
            return out
        if self._num_rate_levels > 0 and self.DEFAULT_RATE_LEVEL_NODE_NAME not in out:
            if self._current_rate_level >= 0:
                out[self.DEFAULT_RATE_LEVEL_NODE_NAME] = self._current_rate_level
            elif force_add_default_dynamic_nodes:
                out[self.DEFAULT_RATE_LEVEL_NODE_NAME] = 0
        if self._num_tasks > 0 and self.DEFAULT_TASK_INDEX_NODE_NAME not in out:
            if self._current_task_idx >= 0:
                out[self.DEFAULT_TASK_INDEX_NODE_NAME] = self._current_task_idx
            elif force_add_default_dynamic_nodes:
                out[self.DEFAULT_TASK_INDEX_NODE_NAME] = 0
        if self._num_complex_levels > 0 and self.DEFAULT_COMPLEX_LEVEL_NODE_NAME not in out:
            if self.complexity_level_greedy_search and self._levels_valid() and not self._searching:
                out.update(**self._complexity_param_all_levels[self._current_complex_level]())  # :673-675
            elif self._current_complex_level >= 0:
                out[self.DEFAULT_COMPLEX_LEVEL_NODE_NAME] = self._current_complex_level
            elif force_add_default_dynamic_nodes:
                out[self.DEFAULT_COMPLEX_LEVEL_NODE_NAME] = 0
        return out

    # ---- shared encoder/decoder constants (latent_graph.py:686-719)
    def _node_generate_process(self, **kwargs):
        out = dict(**kwargs)
        sym = self.DEFAULT_EDGE_SPLIT_SYMBOL
        for name, module in self.node_generators.items():
            inputs = {ik: out[nk] for nk, ik in self.node_generator_input_mapping.get(name, {}).items()}
            if sym in name:
                inode, onode = name.split(sym)
                if onode in out:
                    continue
                if name in out:
                    out[onode] = out.pop(name)
                    continue
                out[onode] = module(out[inode], **inputs)
            elif name not in out:
                out[name] = module(**inputs)
        return out

    # ---- inference pass (latent_graph.py:721-758)
    def _inference_process(self, input_dict):
        out = dict(**input_dict)
        sym = self.DEFAULT_EDGE_SPLIT_SYMBOL
        for node in self.latent_node_inference_topo_order:
            kw = {ik: out[nk] for nk, ik in self.latent_inference_input_mapping.get(node, {}).items()}
            for edge in self._inference_edges_into[node]:
                kw.update({ik: out[ek] for ek, ik in self.latent_inference_input_mapping.get(edge, {}).items()})
                inode, onode = edge.split(sym)
                with self.profiler.start_time_profile(f"latent_inference_modules_{edge}"):
                    val = self.latent_inference_modules[edge](out[inode], **kw)
                if onode in out:   # a second edge into the node: collect (latent_graph.py:741-746)
                    if not isinstance(out[onode], list):
                        out[onode] = [out[onode]]
                    out[onode].append(val)
                else:
                    out[onode] = val
            if node in self.latent_inference_node_aggregator_modules:   # (:748-749)
                out[node] = self.latent_inference_node_aggregator_modules[node](out[node])
        return out

    # ---- generative pass (latent_graph.py:760-868)
    def _generative_process(self, input_dict, prior_dict=None, do_encode=False, coder_kwargs=None, **kwargs):
        """``coder_kwargs``: {node: keywords} handed to that node's entropy coder alone (the quantiser step of the y coder) --
        not an input of the graph: no mapping, module or node generator sees them."""
        coder_kwargs = coder_kwargs or {}
        data = dict(**input_dict)
        kw_all = dict(**input_dict, **kwargs)
        prior_dict = dict(prior_dict or {})
        sym = self.DEFAULT_EDGE_SPLIT_SYMBOL
        nodes = list(self.latent_node_generative_topo_order)
        if do_encode and self.use_lossy_compression:
            nodes.remove(self.DEFAULT_INPUT_NODE_NAME)
        for node in nodes:
            prior_dict.setdefault(node, dict())
            if node in self.latent_generative_node_aggregator_modules:
                # (:795-796) the reference replaces the node's prior DICT by the aggregator's result and then goes on treating it
                # as a dict (len(), .values(), :806-819): only an aggregator that returns a mapping works there; same here
                agg = self.latent_generative_node_aggregator_modules[node](list(prior_dict[node].values()))
                if not isinstance(agg, dict):
                    raise TypeError(f"latent_generative_node_aggregator of node {node} must return a dict of priors "
                                    "(the reference's own traversal reads .values() of the result, latent_graph.py:806-819)")
                prior_dict[node] = agg
            node_data = data.get(node)
            if node in self.latent_node_entropy_coders:
                coder = self.latent_node_entropy_coders[node]
                pk = dict()
                priors = prior_dict[node]
                if node in self.latent_generative_input_mapping:
                    for nk, ik in self.latent_generative_input_mapping[node].items():
                        if len(priors) == 1:
                            pk.update(prior=list(priors.values())[0])
                        if nk in priors:
                            pk[ik] = priors[nk]
                        elif nk in kw_all:
                            pk[ik] = kw_all[nk]
                        else:
                            raise ValueError(f"latent_generative_input_mapping incorrect! node {node}, mapping {nk} : {ik}")
                else:
                    assert len(priors) <= 1
                    if len(priors) == 1:
                        pk.update(prior=list(priors.values())[0])
                pk.update(coder_kwargs.get(node, {}))
                if do_encode and pk.get("rate_target") is not None:   # the budget covers what the image's earlier streams spent
                    pk["rate_target"].extra_words = self._words_coded(data, nodes[:nodes.index(node)], node_data.shape[0])
                with self.profiler.start_time_profile(f"latent_node_entropy_coders_{node}"):
                    if isinstance(node_data, (bytes, memoryview)):
                        node_data = coder.decode(node_data, **pk)
                        data[node] = node_data
                    else:
                        raw = node_data
                        # forward: quantised latent (:836).  When encoding, a node whose quantised value feeds no
                        # further module (the last latent: its only edge is the synthesis transform, skipped
                        # below) does not need it, and nobody reads the rate estimate either.
                        feeds = [e for e in self._generative_edges_from[node]
                                 if not (do_encode and self.use_lossy_compression and e.split(sym)[1] == self.DEFAULT_INPUT_NODE_NAME)]
                        if do_encode and not feeds:
                            node_data = None
                        else:
                            node_data = coder(raw, **pk)
                        if do_encode:  # (:838); coders that can, only enqueue their GPU work here (resolved in encode())
                            data[node] = coder.encode(raw, lazy=True, **pk) if getattr(coder, "supports_lazy_encode", False) \
                                else coder.encode(raw, **pk)
                        else:
                            data[node] = node_data
                    kw_all[node] = node_data
            for edge in self._generative_edges_from[node]:
                ek = {ik: kw_all[k] for k, ik in self.latent_generative_input_mapping.get(edge, {}).items()}
                inode, onode = edge.split(sym)
                if do_encode and self.use_lossy_compression and onode == self.DEFAULT_INPUT_NODE_NAME:
                    continue  # g_s is not needed to encode (:855-856)
                with self.profiler.start_time_profile(f"latent_generative_modules_{edge}"):
                    val = self.latent_generative_modules[edge](node_data, **ek)
                kw_all[edge] = val
                prior_dict.setdefault(onode, dict())[inode] = val
        return data, prior_dict

    def _coded_nodes(self):
        nodes = list(self.latent_node_generative_topo_order)
        if self.use_lossy_compression:
            nodes.remove(self.DEFAULT_INPUT_NODE_NAME)
        return nodes

    # ---- fused C entry points for the plain hyperprior graph (include/basic_hip.h section 8)
    use_fused_session = True    # set False to force the module-by-module path (the two give identical bytes: tests)
    fused_rans_waves = 0        # wavefronts (image streams) per workgroup of the session's rANS launches; 0 = library default
    fused_transform_token = False   # order the transform phases of all such sessions in GPU time (stream workers): True / 1 = one at a time, 2 = two at a time

    def _fused_session(self, kwargs, prior):
        """The HyperpriorSession serving this graph, or None when the graph is anything but
        x -g_a-> y -h_a-> z, z: EntropyBottleneck coder, y: GaussianConditional coder (or its mean-scale form) on h_s(z), x: dummy
        (configs/lossy_graph_scalable_exp_hp.py:182-215) with no dynamic nodes / gains / caller-supplied inputs.  The session tells
        the two y coders apart by the channels h_s ends in."""
        if not self.use_fused_session or self.training or prior is not None or kwargs:
            return None
        elig = getattr(self, "_fused_eligible", None)
        if elig is None:
            from ..prior_model.prior_coder.compressai_coder import (CompressAIEntropyBottleneckPriorCoder,
                                                                    CompressAIGaussianConditionalCoder,
                                                                    CompressAIMeanScaleGaussianConditionalCoder)
            from ...nn.models.google import BasicHyperpriorModule
            c, inf, gen = self.latent_node_entropy_coders, self.latent_inference_modules, self.latent_generative_modules
            elig = (list(self.latent_node_inference_topo_order) == ["x", "y", "z"]
                    and list(self.latent_node_generative_topo_order) == ["z", "y", "x"]
                    and len(self.node_generators) == 0 and self._num_rate_levels <= 0 and self._num_complex_levels <= 0
                    and self._num_tasks <= 0 and set(inf.keys()) == {"x_y", "y_z"} and set(gen.keys()) == {"z_y", "y_x"}
                    and all(type(m).forward is BasicHyperpriorModule.forward for m in list(inf.values()) + list(gen.values()))
                    and type(c["y"]) in (CompressAIGaussianConditionalCoder, CompressAIMeanScaleGaussianConditionalCoder)
                    and type(c["z"]) is CompressAIEntropyBottleneckPriorCoder
                    and not self.latent_inference_input_mapping and not self.latent_generative_input_mapping
                    and (self.use_lossy_compression or isinstance(c["x"] if "x" in c else None, LossyDummyEntropyCoder)))
            self._fused_eligible = bool(elig)
        if not elig:
            return None
        c, inf, gen = self.latent_node_entropy_coders, self.latent_inference_modules, self.latent_generative_modules
        zc, yc = c["z"], c["y"]
        zc._ready()
        yc._ready()
        plans = [m.plans() for m in (inf["x_y"], inf["y_z"], gen["z_y"], gen["y_x"])]
        key = tuple(p._h.value for pl in plans for p in pl) + (zc._tables._h.value, yc._tables._h.value)
        sess = getattr(self, "_fused", None)
        if sess is None or sess.key != key:
            from ...nn import kernels as K
            sess = K.HyperpriorSession(*plans, zc.entropy_bottleneck.medians(), zc._tables, yc.scale_table, yc.scale_bound, yc._tables)
            self._fused = sess
        if getattr(sess, "_waves", 0) != self.fused_rans_waves:
            sess.set_rans_waves(self.fused_rans_waves)
            sess._waves = self.fused_rans_waves
        if getattr(sess, "_lanes", 1) != yc.stream_lanes:   # the y coder's lane streams: the two paths write the same bytes
            sess.set_stream_lanes(yc.stream_lanes)
            sess._lanes = yc.stream_lanes
        if getattr(sess, "_token", False) != self.fused_transform_token:
            sess.set_transform_token(self.fused_transform_token)
            sess._token = self.fused_transform_token
        return sess

    QSTEP_NODE = "y"   # the node whose coder takes the quantiser step

    def _words_coded(self, data, nodes, batch):
        """32-bit words per image in the bodies of ``nodes`` coded so far (host code; a pending body is synchronised for its lengths)."""
        from ...nn import kernels as K
        total = np.zeros(batch, dtype=np.int64)
        for n in nodes:
            body = data.get(n)
            if hasattr(body, "_end"):
                off = body._end()[1]
            elif isinstance(body, (bytes, memoryview)) and len(body) >= 12:
                off = K.unframe_streams(bytes(body))[1]
            else:
                continue
            words = np.diff(np.asarray(off, dtype=np.int64))
            if words.size % batch:
                raise ValueError(f"node {n} holds {words.size} streams, no multiple of the batch of {batch}")
            total += words.reshape(batch, -1).sum(1)
        return total.astype(np.int32)

    def payload_bytes(self, data, batch):
        """Bytes of rANS payload per image in a coded string of ``batch`` images: the streams of every coded node, without the
        framing (headers, one uint32 length per stream).  Host code, for coders that write stream bodies (write_body)."""
        nodes = self._coded_nodes()
        bodies = dict(zip(nodes, (bytes(v) for v in split_merged_views(data, num_segments=len(nodes)))))
        return 4 * self._words_coded(bodies, nodes, batch).astype(np.int64)

    def _rate_coder_kwargs(self, rate_target, batch):
        """``rate_target`` of encode -> (RateTarget, the keywords of the y coder), or (None, None) without one; TypeError when the
        graph's y coder is not the GaussianConditional coder, ValueError for an invalid request (utils/rate.py)."""
        if rate_target is None:
            return None, None
        from ..prior_model.prior_coder.compressai_coder import (CompressAIGaussianConditionalCoder,
                                                                CompressAIMeanScaleGaussianConditionalCoder)
        from ...utils.rate import as_rate_target
        coder = self.latent_node_entropy_coders[self.QSTEP_NODE] if self.QSTEP_NODE in self.latent_node_entropy_coders else None
        if type(coder) not in (CompressAIGaussianConditionalCoder, CompressAIMeanScaleGaussianConditionalCoder):
            raise TypeError(f"rate_target= chooses the quantiser step of a CompressAIGaussianConditionalCoder (scale-only or mean-scale) at node '{self.QSTEP_NODE}'; "
                            f"this graph codes it with {type(coder).__name__}")
        rt = as_rate_target(rate_target, batch)
        return rt, {self.QSTEP_NODE: dict(rate_target=rt)}

    def _qstep_coder_kwargs(self, qstep, batch):
        """``qstep`` of encode / decode -> (validated float32 steps, the keywords of the y coder), or (None, None) without one.
        TypeError when the graph's y coder is not the GaussianConditional coder; ValueError for invalid steps (utils/qstep.py)."""
        if qstep is None:
            return None, None
        from ..prior_model.prior_coder.compressai_coder import (CompressAIGaussianConditionalCoder,
                                                                CompressAIMeanScaleGaussianConditionalCoder)
        coder = self.latent_node_entropy_coders[self.QSTEP_NODE] if self.QSTEP_NODE in self.latent_node_entropy_coders else None
        if type(coder) not in (CompressAIGaussianConditionalCoder, CompressAIMeanScaleGaussianConditionalCoder):
            raise TypeError(f"qstep= is the quantiser step of a CompressAIGaussianConditionalCoder (scale-only or mean-scale) at node '{self.QSTEP_NODE}'; this "
                            f"graph codes it with {type(coder).__name__}.  The PGM coders' own knob is "
                            "quantizer_type='uniform_scale' with quantizer_params=[step]")
        steps = check_qsteps(qstep, batch)
        return steps, {self.QSTEP_NODE: dict(qstep=steps)}

    def _skip_coder_kwargs(self, skip_rows):
        """``skip_rows`` of encode / decode -> the validated row count, or None without one.  TypeError when the graph's y coder is
        not the GaussianConditional coder; ValueError for an invalid count (utils/skip.py)."""
        if skip_rows is None:
            return None
        from ..prior_model.prior_coder.compressai_coder import (CompressAIGaussianConditionalCoder,
                                                                CompressAIMeanScaleGaussianConditionalCoder)
        from ...utils.skip import SKIP_TABLE_ROWS, check_skip_rows
        coder = self.latent_node_entropy_coders[self.QSTEP_NODE] if self.QSTEP_NODE in self.latent_node_entropy_coders else None
        if type(coder) not in (CompressAIGaussianConditionalCoder, CompressAIMeanScaleGaussianConditionalCoder):
            raise TypeError(f"skip_rows= is skip coding of a CompressAIGaussianConditionalCoder (scale-only or mean-scale) at node '{self.QSTEP_NODE}'; "
                            f"this graph codes it with {type(coder).__name__}, whose context model reads every symbol: skip coding of the "
                            "autoregressive codecs is not implemented")
        return check_skip_rows(skip_rows, coder.scale_table.numel() or SKIP_TABLE_ROWS)

    @staticmethod
    def _no_skip_rows(kwargs, what):
        if "skip_rows" in kwargs:
            raise ValueError(f"{what} takes no skip_rows=: skip coding of tiled pictures is not implemented (their containers carry no "
                             "skip rows); code the picture whole with compress_skip")

    def _qstep_stream_batch(self, data):
        """Images in a coded string, from the y body's header (host code: nothing is launched)."""
        nodes = self._coded_nodes()
        body = split_merged_views(data, num_segments=len(nodes))[nodes.index(self.QSTEP_NODE)]
        if len(body) < 12:
            raise ValueError("truncated stream: the y body has no header")
        ns = struct.unpack(">3I", body[:12])[2]
        lanes = self.latent_node_entropy_coders[self.QSTEP_NODE].stream_lanes
        if ns < lanes or ns % lanes:
            raise ValueError(f"the y body holds {ns} streams, no multiple of this coder's {lanes} stream lanes")
        return ns // lanes

    def encode(self, data, *args, prior=None, qstep=None, rate_target=None, skip_rows=None, **kwargs):
        """``qstep``: None -- today's codec; a number or one number per image -- the quantiser step of the y coder (INTEGRATION.md
        "Quantiser step").  Like ``output_dtype`` of decode() it is not one of ``kwargs``: it neither changes the path a call takes
        nor reaches a node generator, and both paths write the same bytes.  The string does not hold the steps: decode() needs them.
        ``skip_rows``: None -- today's codec; r -- skip coding of the y coder (INTEGRATION.md "Skip coding"), an explicit keyword in the
        same way, with ``qstep=`` or alone; decode() needs it too."""
        steps, coder_kwargs = self._qstep_coder_kwargs(qstep, data.shape[0])
        rt, rate_kwargs = self._rate_coder_kwargs(rate_target, data.shape[0])
        skip = self._skip_coder_kwargs(skip_rows)
        if rt is not None:
            if steps is not None:
                raise ValueError("rate_target= and qstep= are two ways to state the step: give one of them")
            if skip is not None:
                raise ValueError("rate_target= and skip_rows= do not combine: the rate curve would count symbols that are not coded")
            coder_kwargs = rate_kwargs
        if skip is not None:
            coder_kwargs = {self.QSTEP_NODE: dict((coder_kwargs or {}).get(self.QSTEP_NODE, {}), skip_rows=skip)}
        with torch.no_grad():
            sess = self._fused_session(kwargs, prior) if not args else None
            if sess is not None:   # one C call: upload (when the batch is on the host), transforms, entropy stage, framing
                if data.is_cuda and data.device != self.device:
                    data = data.to(device=self.device)
                with self.profiler.start_time_profile("encode_fused"):
                    if rt is not None:   # the steps are chosen inside the call; the choices come back with the stream lengths
                        sess.set_rate_targets(rt.budgets, rt.candidates, rt.passes)
                        try:
                            out = sess.encode(data)
                            rt.set_result(*sess.rate_result(data.shape[0]))
                        finally:
                            sess.set_rate_targets(None)
                    elif steps is None and not skip:
                        out = sess.encode(data)
                    else:
                        if steps is not None:
                            sess.set_qsteps(steps)
                        try:
                            sess.set_skip_rows(skip)
                            out = sess.encode(data)
                        finally:
                            sess.set_skip_rows(0)
                            sess.set_qsteps(None)
                if self.after_inference_hook is not None:
                    self.after_inference_hook()
                return out
            if data.device != self.device:
                data = data.to(device=self.device)
            if data.dtype == torch.uint8:   # an 8-bit image batch: uploaded as bytes, converted in front of the first layer
                from ...nn import kernels as K
                data = K.image_u8_to_f32(data)
            node_dict = self._node_generate_process(**self._get_default_node_dict(force_add_default_dynamic_nodes=True, **kwargs))
            input_dict = {self.DEFAULT_INPUT_NODE_NAME: data, **node_dict}
            prior_dict = dict() if prior is None else {self.DEFAULT_INPUT_NODE_NAME: dict(prior=prior)}
            with self.profiler.start_time_profile("encode_inference"):
                latent_dict = self._inference_process(input_dict)
            if self.after_inference_hook is not None:   # the analysis transforms are enqueued (see stream_workers.py)
                self.after_inference_hook()
            with self.profiler.start_time_profile("encode_generative"):
                data_dict, _ = self._generative_process(latent_dict, prior_dict=prior_dict, do_encode=True, coder_kwargs=coder_kwargs)
            nodes = self._coded_nodes()
            bodies = [data_dict[n] for n in nodes]
            if any(hasattr(b, "write_into") for b in bodies):
                out = merge_bodies(bodies)  # = merge_bytes(..., num_segments=len(nodes)), bodies framed in place
            else:
                bodies = [b.result() if hasattr(b, "result") else b for b in bodies]
                out = merge_bytes(bodies, num_segments=len(nodes))
            if rt is not None:
                rt.resolve()
            return out

    def decode(self, data, *args, prior=None, output_dtype=None, qstep=None, skip_rows=None, **kwargs):
        """``output_dtype``: None / torch.float32 -- the reconstruction as the graph gives it; torch.uint8 -- the picture,
        ``nan_to_num(x, nan=0).clamp(0, 1).mul(255).round()`` as bytes, converted on the device.  The keyword is the caller's
        wish about the RESULT: it is not one of ``kwargs``, so it neither changes the path a call takes nor reaches a node generator.
        ``qstep``: the steps encode() was given (one, or one per image of the string), an explicit keyword in the same way.
        ``skip_rows``: the rows encode() was given, likewise."""
        if output_dtype not in (None, torch.float32, torch.uint8):
            raise TypeError(f"output_dtype is torch.float32 or torch.uint8, not {output_dtype}")
        steps, coder_kwargs = self._qstep_coder_kwargs(qstep, None)
        skip = self._skip_coder_kwargs(skip_rows)
        if skip is not None:
            coder_kwargs = {self.QSTEP_NODE: dict((coder_kwargs or {}).get(self.QSTEP_NODE, {}), skip_rows=skip)}
        if steps is not None:   # one step or one per image, checked against the string's own header before anything is launched
            check_qsteps(steps, self._qstep_stream_batch(data))
        with torch.no_grad():
            sess = self._fused_session(kwargs, prior) if not args else None
            if sess is not None:
                with self.profiler.start_time_profile("decode_fused"):
                    if steps is None and not skip:
                        return sess.decode(data, device=self.device, output_dtype=output_dtype or torch.float32)
                    if steps is not None:
                        sess.set_qsteps(steps)
                    try:
                        sess.set_skip_rows(skip)
                        return sess.decode(data, device=self.device, output_dtype=output_dtype or torch.float32)
                    finally:
                        sess.set_skip_rows(0)
                        sess.set_qsteps(None)
            node_dict = self._node_generate_process(**self._get_default_node_dict(force_add_default_dynamic_nodes=True, **kwargs))
            nodes = self._coded_nodes()
            # coders that read their stream through the buffer protocol get it in place; others get bytes
            segs = split_merged_views(data, num_segments=len(nodes))
            input_dict = {n: (v if getattr(self.latent_node_entropy_coders[n], "accepts_buffer", False) else v.tobytes())
                          for n, v in zip(nodes, segs)}
            prior_dict = dict() if prior is None else {self.DEFAULT_INPUT_NODE_NAME: dict(prior=prior)}
            if self.use_lossy_compression:
                input_dict[self.DEFAULT_INPUT_NODE_NAME] = b""
            with self.profiler.start_time_profile("decode_generative"):
                data_dict, _ = self._generative_process(input_dict, prior_dict=prior_dict, coder_kwargs=coder_kwargs, **node_dict)
            out = data_dict[self.DEFAULT_INPUT_NODE_NAME]
            if output_dtype == torch.uint8:
                from ...nn import kernels as K
                out = K.image_f32_to_u8(out)
            return out

    # ---- coalesced items: N batch-1 items coded in chip-filling calls, every item keeping the bytes of its own batch-1 call
    last_items_calls = 0   # encode() / decode() calls the last encode_items() / decode_items() made

    def _items_ctx(self, node, node_dict):
        """What the graph knows about a coded node and its coder's framing may depend on: whether the node is coded under a prior
        (the PGM coders then write no shape head) and the controller values mapped onto the coder's arguments (``blend_weight``)."""
        sym = self.DEFAULT_EDGE_SPLIT_SYMBOL
        ctx = dict(has_prior=any(e.split(sym)[1] == node for e in self.latent_generative_modules))
        for nk, ik in self.latent_generative_input_mapping.get(node, {}).items():
            if nk in node_dict:
                ctx[ik] = node_dict[nk]
        return ctx

    def _items_framing(self):
        """[(coder, ctx)] of the coded nodes in stream order, or None when one of them cannot give every image its own body."""
        node_dict = self._node_generate_process(**self._get_default_node_dict(force_add_default_dynamic_nodes=True))
        out = []
        for node in self._coded_nodes():
            coder = self.latent_node_entropy_coders[node]
            if not (hasattr(coder, "split_items") and hasattr(coder, "merge_items") and getattr(coder, "can_split_items", False)):
                return None
            out.append((coder, self._items_ctx(node, node_dict)))
        return out

    @staticmethod
    def _split_string(data, n, framing):
        """The n batch-1 strings of a batch's string, node by node (framing: _items_framing())."""
        return item_framing.split_codec_string(data, n, [(lambda body, k, c=c, ctx=ctx: c.split_items(body, k, **ctx)) for c, ctx in framing])

    @staticmethod
    def _merge_strings(strings, framing):
        """Inverse of _split_string: batch-1 strings -> the string of the batch of them."""
        return item_framing.merge_codec_strings(strings, [(lambda bodies, c=c, ctx=ctx: c.merge_items(bodies, **ctx)) for c, ctx in framing])

    @staticmethod
    def _check_item(x):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[0] != 1:
            raise ValueError("an item is a [1, C, H, W] tensor" + (f", not {tuple(x.shape)}" if isinstance(x, torch.Tensor) else ""))

    def encode_items(self, items, *args, max_batch=None, **kwargs) -> List[bytes]:
        """N batch-1 items -> their N byte strings, EXACTLY what ``[self.encode(x) for x in items]`` returns, from as few encode()
        calls as the shapes allow: items of one shape share a batch (utils/item_framing.coalesce_chunks), the batch's string is split
        node by node.  One call per item when there is nothing to share, a coder cannot split, or the call brings arguments."""
        items = list(items)
        for x in items:
            self._check_item(x)
        self.last_items_calls = 0
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        if framing is None:
            chunks = [[i] for i in range(len(items))]
        else:
            chunks = item_framing.coalesce_chunks([(tuple(x.shape), x.dtype) for x in items], max_batch)
        out = [None] * len(items)
        for chunk in chunks:
            self.last_items_calls += 1
            if len(chunk) == 1:
                out[chunk[0]] = self.encode(items[chunk[0]], *args, **kwargs)
                continue
            first = items[chunk[0]]
            # the chunk's ONE device batch, filled item by item on the current stream (no host-side stack of the items); uint8 items
            # whose memory is [H][W][C], as an image decoder leaves them, are gathered in that order (plain copies) and converted once
            from ...nn.kernels import image_layout_of
            if first.dtype == torch.uint8 and all(image_layout_of(items[i]) == "hwc" for i in chunk):
                _, C, H, W = first.shape
                batch = torch.empty((len(chunk), H, W, C), dtype=first.dtype, device=self.device).permute(0, 3, 1, 2)
            else:
                batch = torch.empty((len(chunk),) + tuple(first.shape[1:]), dtype=first.dtype, device=self.device)
            for j, i in enumerate(chunk):
                batch[j:j + 1].copy_(items[i], non_blocking=True)
            for i, one in zip(chunk, self._split_string(self.encode(batch), len(chunk), framing)):
                out[i] = one
        return out

    def decode_items(self, strings, *args, max_batch=None, output_dtype=None, **kwargs) -> List[torch.Tensor]:
        """N batch-1 strings -> their N reconstructions ([1, C, H, W] views of the batches' outputs, in input order), each equal to
        ``self.decode(string)``.  Strings share a call when the shapes their own headers state agree on every node (a body without
        a header, the AR body under an aligned prior, follows the others)."""
        strings = list(strings)
        self.last_items_calls = 0
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        if framing is None:
            chunks = [[i] for i in range(len(strings))]
        else:
            keys = []
            for s in strings:
                segs = split_merged_bytes(bytes(s), num_segments=len(framing))
                keys.append(tuple(c.item_shape(seg, **ctx) if hasattr(c, "item_shape") else None for (c, ctx), seg in zip(framing, segs)))
            chunks = item_framing.coalesce_chunks(keys, max_batch)
        out = [None] * len(strings)
        for chunk in chunks:
            self.last_items_calls += 1
            if len(chunk) == 1:
                out[chunk[0]] = self.decode(strings[chunk[0]], *args, output_dtype=output_dtype, **kwargs)
                continue
            rec = self.decode(self._merge_strings([strings[i] for i in chunk], framing), output_dtype=output_dtype)
            for j, i in enumerate(chunk):
                out[i] = rec[j:j + 1]
        return out

    # ---- tiled pictures: one picture coded as independent tiles, every tile keeping the bytes of its own batch-1 call
    last_tiles_decoded = 0   # tiles the last decode_tiled() decoded

    @staticmethod
    def _tile_size(tile):
        th, tw = (tile, tile) if isinstance(tile, int) else tuple(tile)
        return int(th), int(tw)

    @staticmethod
    def _padded_tile(picture, y, x, h, w):
        """``picture[:, :, y:y + h, x:x + w]`` of a ``[1, C, H, W]`` picture; where the rectangle leaves the picture at the bottom or right,
        the last row and column replicated: sample (r, q) is ``picture[..., min(y + r, H - 1), min(x + q, W - 1)]`` (index tensors)."""
        H, W = picture.shape[2], picture.shape[3]
        if y + h <= H and x + w <= W:
            return picture[:, :, y:y + h, x:x + w]
        iy = torch.arange(y, y + h, device=picture.device).clamp_(max=H - 1)
        ix = torch.arange(x, x + w, device=picture.device).clamp_(max=W - 1)
        return picture[:, :, iy[:, None], ix[None, :]]

    def _pooled_batches(self, pictures, grids, max_batch):
        """The pooled plan over ``pictures`` (on the device): yields (refs, batch) per chunk of utils.tiling.pool_tiles, uint8 pictures
        first -- ``refs`` the chunk's PooledTiles with ``picture`` an index into ``pictures``, ``batch`` the one tile as it is cut out of
        its picture (a chunk of one) or the chunk's float32 batch (uint8 tiles cut by one image_tiles_gather launch)."""
        from ...nn import kernels as K
        from ...utils import tiling
        for dtype in (torch.uint8, torch.float32):
            own = [p for p, x in enumerate(pictures) if x.dtype == dtype]
            padded = any(grids[p].pad_to != (1, 1) for p in own)
            for chunk in tiling.pool_tiles([grids[p] for p in own], max_batch):
                refs = [t._replace(picture=own[t.picture]) for t in chunk.tiles]
                if len(refs) == 1:
                    p, k, y, x = refs[0]
                    batch = self._padded_tile(pictures[p], y, x, chunk.h, chunk.w)
                elif dtype == torch.uint8:
                    batch = K.image_tiles_gather(pictures, refs, chunk.h, chunk.w, pad=padded)
                else:
                    batch = torch.empty((len(refs), pictures[own[0]].shape[1], chunk.h, chunk.w), dtype=dtype, device=self.device)
                    for j, (p, _, y, x) in enumerate(refs):
                        batch[j].copy_(self._padded_tile(pictures[p], y, x, chunk.h, chunk.w)[0])
                yield refs, batch

    def _encode_pooled(self, pictures, grids, framing, max_batch, args=(), kwargs=None, steps=None):
        """The tile strings of ``pictures`` (on the device) over ``grids``, ``[picture][tile]``: the pooled plan (utils.tiling.pool_tiles)
        when ``framing`` splits a batch's string, one encode() per tile otherwise.  Counts into ``last_items_calls``.
        ``steps[p]``: float32, the quantiser step of every tile of picture p; a chunk's steps reach its encode() as ``qstep=``, an
        explicit keyword, so they change neither the plan nor the number of calls."""
        kwargs = kwargs or {}
        strings = [[None] * len(g) for g in grids]
        with torch.no_grad(), torch.cuda.device(self.device):
            if framing is None:
                for p, g in enumerate(grids):
                    for k in range(len(g)):
                        y, x, _, _ = g.tile_rect(k)
                        self.last_items_calls += 1
                        strings[p][k] = self.encode(self._padded_tile(pictures[p], y, x, *g.coded_size(k)), *args, **kwargs)
                return strings
            for refs, batch in self._pooled_batches(pictures, grids, max_batch):
                self.last_items_calls += 1
                stated = {} if steps is None else dict(qstep=np.array([steps[p][k] for p, k, _, _ in refs], dtype=np.float32))
                if len(refs) == 1:
                    strings[refs[0].picture][refs[0].index] = self.encode(batch, **stated)
                    continue
                for (p, k, _, _), one in zip(refs, self._split_string(self.encode(batch, **stated), len(refs), framing)):
                    strings[p][k] = one
        return strings

    def encode_tiled(self, image, *args, tile=(512, 512), max_batch=None, overlap=0, pad_to=1, **kwargs) -> bytes:
        """One picture ``[1, C, H, W]`` (uint8 in chw or hwc memory, or float32; host or device) -> the container of its tiles'
        strings (utils/tiling.py), tile k's string EXACTLY ``self.encode(image[:, :, y:y + h, x:x + w])``.  Tiles of one size are cut
        out of the uint8 picture by one kernel launch per chunk of at most ``max_batch`` and coded in one encode() call, whose string
        is split as in encode_items; one call per tile when a coder cannot split, a chunk holds one tile, or the call brings
        arguments.  Tiles are coded independently.  ``overlap`` (an int, or ``(oy, ox)``, at most half a tile): neighbouring tiles
        share that many rows and columns (utils/tiling.py), the container is BTL2, and decode_tiled cross-fades the seams; with 0,
        the default, the tiles abut and every byte of the container is what it was before overlaps existed.
        ``pad_to`` (an int, or ``(py, px)``, dividing the tile): an edge tile is coded at its size rounded up to multiples of py x px, the
        picture's last row and column replicated (utils/tiling.py): tile k's string is EXACTLY ``self.encode(P_k)`` of that padded tile,
        the container is BTL3, and decode_tiled crops.  The tiles then take the pooled plan over this one picture (tiles of one coded
        size share calls of at most ``max_batch``, cut by nn.kernels.image_tiles_gather), so ``pad_to=tile`` codes a picture as one
        group.  With 1, the default, nothing is padded and nothing changes."""
        from ...utils import tiling
        self._no_skip_rows(kwargs, "encode_tiled")
        self._check_picture(image)
        _, C, H, W = image.shape
        grid = tiling.TileGrid(H, W, *self._tile_size(tile), overlap=overlap, pad_to=pad_to)
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        out = self._encode_tiles(image, grid, framing, max_batch, args, kwargs)
        return tiling.pack_tiled(C, H, W, grid.th, grid.tw, out, overlap=grid.overlap, pad_to=grid.pad_to)

    @classmethod
    def _check_picture(cls, image):
        cls._check_item(image)
        if image.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"a picture is torch.uint8 or torch.float32, not {image.dtype}")

    def _encode_tiles(self, image, grid, framing, max_batch, args=(), kwargs=None, steps=None):
        """The tile strings of one picture over ``grid``, by encode_tiled's plan.  ``steps``: float32, one quantiser step per tile --
        ``qstep=`` of the encode() call that codes the tile, an explicit keyword: the plan and ``last_items_calls`` are the step-less
        call's."""
        from ...nn import kernels as K
        from ...utils import tiling
        kwargs = kwargs or {}
        C = image.shape[1]
        self.last_items_calls = 0
        if image.device != self.device:
            image = image.to(device=self.device)   # once, as it lies: a dense picture keeps its strides
        if grid.pad_to != (1, 1):
            out, = self._encode_pooled([image], [grid], framing, max_batch, args, kwargs, steps=None if steps is None else [steps])
            return out
        out = [None] * len(grid)
        with torch.no_grad():
            for group in grid.groups():
                for sub in tiling.split_group(group, 1 if framing is None else max_batch):
                    self.last_items_calls += 1
                    stated = {} if steps is None else dict(qstep=np.ascontiguousarray(steps[list(sub.indices)], dtype=np.float32))
                    if len(sub.indices) == 1:
                        y, x = sub.y0, sub.x0
                        out[sub.indices[0]] = self.encode(image[:, :, y:y + sub.h, x:x + sub.w], *args, **stated, **kwargs)
                        continue
                    if image.dtype == torch.uint8:
                        batch = K.image_tiles_to_f32(image, sub)
                    else:
                        batch = torch.empty((len(sub.indices), C, sub.h, sub.w), dtype=image.dtype, device=self.device)
                        for j in range(len(sub.indices)):
                            y, x = sub.y0 + j // sub.nx * sub.step_y, sub.x0 + j % sub.nx * sub.step_x
                            batch[j].copy_(image[0, :, y:y + sub.h, x:x + sub.w])
                    for k, one in zip(sub.indices, self._split_string(self.encode(batch, **stated), len(sub.indices), framing)):
                        out[k] = one
        return out

    def decode_tiled(self, data, *args, output_dtype=torch.uint8, layout="chw", region=None, max_batch=None, **kwargs):
        """A container of encode_tiled -> the picture ``[1, C, H, W]`` at its own size: every tile's ``self.decode(string)``, cropped
        to the tile and written at its place (``output_dtype`` None / torch.float32), or ``image_f32_to_u8`` of that (torch.uint8:
        converted, cropped and pasted by one kernel launch per chunk).  ``layout`` "hwc": the result's memory is [H][W][C].
        ``region=(y0, x0, y1, x1)``: only the tiles that intersect the rectangle are decoded (``last_tiles_decoded``), and the
        rectangle is returned, equal to that slice of the full result.
        Overlapped tiles (a BTL2 container; the overlap is read from it): the tiles that cover a sample of the picture or region are
        decoded as above, and ONE blend launch (nn.kernels.image_tiles_blend) writes the result from their reconstructions, the
        seams cross-faded as include/basic_hip.h section 8c defines.  The reconstructions of ALL decoded tiles are resident until
        that launch: 4 * C * sh * sw bytes per tile on top of the result, where the abutting path holds one chunk at a time.
        Edge-padded tiles (a BTL3 container; ``pad_to`` is read from it): every tile's reconstruction is cropped to the tile's valid
        rectangle, its top-left.  The tiles of the picture or region take the pooled plan of decode_tiled_items over this one picture
        (one decode() call per coded size and ``max_batch``; uint8 results pasted by nn.kernels.image_tiles_scatter with ``clip=True``);
        overlapped ones are written by the same blend launch, which reads those top-left samples."""
        from ...nn import kernels as K
        self._no_skip_rows(kwargs, "decode_tiled")
        from ...utils import tiling
        if output_dtype not in (None, torch.float32, torch.uint8):
            raise TypeError(f"output_dtype is torch.float32 or torch.uint8, not {output_dtype}")
        if layout not in K.IMAGE_LAYOUTS:
            raise ValueError(f"layout is 'chw' or 'hwc', not {layout!r}")
        head, steps = self._unpack_tiled(data)
        C, H, W, th, tw, overlap, pad_to, strings = head
        grid = tiling.TileGrid(H, W, th, tw, overlap, pad_to)
        if region is None:
            groups, (ry0, rx0, ry1, rx1) = grid.groups(), (0, 0, H, W)
        else:
            ry0, rx0, ry1, rx1 = (int(v) for v in region)
            groups = grid.tiles_of_region(ry0, rx0, ry1, rx1)
        # the canvas covers the decoded tiles: the picture, or the region widened to tile borders
        cy0, cx0 = ry0 // th * th, rx0 // tw * tw
        ch, cw = min(H, -(-ry1 // th) * th) - cy0, min(W, -(-rx1 // tw) * tw) - cx0
        self.last_items_calls = self.last_tiles_decoded = 0
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        as_u8 = output_dtype == torch.uint8
        blend = overlap != (0, 0)
        if blend:   # the result is the rectangle itself: the blend launch writes nothing else
            cy0, cx0, ch, cw = ry0, rx0, ry1 - ry0, rx1 - rx0
        recs = []
        with torch.no_grad(), torch.cuda.device(self.device):
            dtype = torch.uint8 if as_u8 else torch.float32
            if layout == "hwc":
                canvas = torch.empty((1, ch, cw, C), dtype=dtype, device=self.device).permute(0, 3, 1, 2)
            else:
                canvas = torch.empty((1, C, ch, cw), dtype=dtype, device=self.device)
            if grid.pad_to != (1, 1):
                self._decode_pooled([head], [grid], [canvas], framing, max_batch, as_u8, picks=[{k for g in groups for k in g.indices}],
                                    origins=[(cy0, cx0)], regions=[(ry0, rx0, ry1, rx1)], args=args, kwargs=kwargs, steps=[steps])
                groups = []
            for group in groups:
                for sub in tiling.split_group(group, 1 if framing is None else max_batch):
                    self.last_items_calls += 1
                    self.last_tiles_decoded += len(sub.indices)
                    stated = {} if steps is None else dict(qstep=np.ascontiguousarray(steps[list(sub.indices)], dtype=np.float32))
                    if len(sub.indices) == 1:
                        rec = self.decode(strings[sub.indices[0]], *args, **stated, **kwargs)
                    else:
                        rec = self.decode(self._merge_strings([strings[k] for k in sub.indices], framing), **stated)
                    if rec.dim() != 4 or rec.shape[0] != len(sub.indices) or rec.shape[1] != C or rec.shape[2] < sub.h or rec.shape[3] < sub.w:
                        raise ValueError(f"tiles of [{len(sub.indices)}, {C}, {sub.h}, {sub.w}] decoded to {tuple(rec.shape)}")
                    if blend:
                        recs.append((rec, sub.indices))
                        continue
                    sub = sub._replace(y0=sub.y0 - cy0, x0=sub.x0 - cx0)
                    if as_u8:
                        K.image_tiles_from_f32(rec, canvas, sub)
                    else:
                        for j in range(len(sub.indices)):
                            y, x = sub.y0 + j // sub.nx * sub.step_y, sub.x0 + j % sub.nx * sub.step_x
                            canvas[0, :, y:y + sub.h, x:x + sub.w].copy_(rec[j, :, :sub.h, :sub.w])
            if blend and grid.pad_to == (1, 1):
                K.image_tiles_blend(recs, grid, canvas, (ry0, rx0, ry1, rx1))
        if region is None:
            return canvas
        return canvas[:, :, ry0 - cy0:ry1 - cy0, rx0 - cx0:rx1 - cx0]

    @staticmethod
    def _unpack_tiled(data):
        """(TiledPicture, steps) of a container, by its magic: BTL1 - BTL3 state no steps (None); BTQ1 states one per tile (float32 [n]),
        validated with the rest of the container before anything is launched (utils/tiling.py)."""
        from ...utils import tiling
        if bytes(data[:4]) == tiling.MAGIC_Q:
            t = tiling.unpack_tiled_q(data)
            return tiling.TiledPicture(*t[:8]), t.steps
        return tiling.unpack_tiled_full(data), None

    def _decode_pooled(self, heads, grids, canvases, framing, max_batch, as_u8, picks=None, origins=None, regions=None, args=(), kwargs=None,
                       steps=None):
        """The pooled decode: the tiles of the containers ``heads`` (utils.tiling.TiledPicture; ``grids`` their TileGrids) decoded in calls
        shared by tiles of one coded size whose strings' own headers agree, each reconstruction cropped to its tile's valid rectangle
        and written into ``canvases[p]``.  ``picks[p]``: the tile numbers of picture p to decode (default: all); ``origins[p]``: where
        canvas p's first sample lies in picture p (default: (0, 0)); ``regions[p]``: the rectangle an overlapped picture's blend launch
        writes (default: the picture; the canvas is then that rectangle).  ``framing`` None: one decode() per tile, with the call's
        arguments.  Counts into ``last_items_calls`` and ``last_tiles_decoded``.  ``steps[p]``: None, or the quantiser steps of picture
        p's tiles (a BTQ1 container); such tiles share calls among themselves only, and a call's steps reach decode() as ``qstep=``."""
        from ...nn import kernels as K
        from ...utils import tiling
        kwargs = kwargs or {}
        steps = steps or [None] * len(heads)
        strings = [t.strings for t in heads]
        blend = [g.overlap != (0, 0) for g in grids]
        # the planner's chunks of one size each, refined by what the strings say about themselves, then cut at max_batch
        chunks = []
        for size in tiling.pool_tiles(grids, None):
            tiles = [t for t in size.tiles if picks is None or t.index in picks[t.picture]]
            if framing is None:
                chunks.extend((size.h, size.w, [t]) for t in tiles)
                continue
            by_key = {}
            for t in tiles:
                segs = split_merged_bytes(strings[t.picture][t.index], num_segments=len(framing))
                key = (heads[t.picture][0], steps[t.picture] is not None) + tuple(c.item_shape(seg, **ctx) if hasattr(c, "item_shape") else None
                                                     for (c, ctx), seg in zip(framing, segs))
                by_key.setdefault(key, []).append(t)
            for tiles in by_key.values():
                step = max_batch or len(tiles)
                chunks.extend((size.h, size.w, tiles[i:i + step]) for i in range(0, len(tiles), step))
        waiting = [0] * len(grids)   # tiles an overlapped picture still lacks
        for h, w, tiles in chunks:
            for t in tiles:
                waiting[t.picture] += blend[t.picture]
        held = [[] for _ in grids]       # its (batch view, tile indices) so far
        for h, w, tiles in chunks:
            self.last_items_calls += 1
            self.last_tiles_decoded += len(tiles)
            stated = {} if steps[tiles[0].picture] is None else dict(qstep=np.array([steps[t.picture][t.index] for t in tiles], dtype=np.float32))
            if len(tiles) == 1:
                rec = self.decode(strings[tiles[0].picture][tiles[0].index], *args, **stated, **kwargs)
            else:
                rec = self.decode(self._merge_strings([strings[t.picture][t.index] for t in tiles], framing), **stated)
            C = heads[tiles[0].picture][0]
            if rec.dim() != 4 or rec.shape[0] != len(tiles) or rec.shape[1] != C or rec.shape[2] < h or rec.shape[3] < w:
                raise ValueError(f"tiles of [{len(tiles)}, {C}, {h}, {w}] decoded to {tuple(rec.shape)}")
            plain = [j for j, t in enumerate(tiles) if not blend[t.picture]]
            if origins is None:
                placed = [tiles[j] for j in plain]
            else:   # the canvas is a window of the picture
                placed = [tiles[j]._replace(y0=tiles[j].y0 - origins[tiles[j].picture][0], x0=tiles[j].x0 - origins[tiles[j].picture][1])
                          for j in plain]
            if plain and as_u8:
                part = rec if len(plain) == len(tiles) else rec[torch.tensor(plain, device=rec.device)]
                # a padded tile leaves its canvas where it leaves its picture: only the valid rectangle is written
                K.image_tiles_scatter(part, canvases, placed, h, w, clip=any(grids[t.picture].pad_to != (1, 1) for t in placed))
            elif plain:
                for j, (p, k, y, x) in zip(plain, placed):
                    _, _, vh, vw = grids[p].tile_rect(k)
                    canvases[p][0, :, y:y + vh, x:x + vw].copy_(rec[j, :, :vh, :vw])
            j = 0
            while j < len(tiles):   # picture-major: an overlapped picture's tiles of this chunk are one slice of the batch
                p, e = tiles[j].picture, j + 1
                while e < len(tiles) and tiles[e].picture == p:
                    e += 1
                if blend[p]:
                    held[p].append((rec[j:e], [t.index for t in tiles[j:e]]))
                    waiting[p] -= e - j
                    if waiting[p] == 0:
                        K.image_tiles_blend(held[p], grids[p], canvases[p], None if regions is None else regions[p])
                        held[p] = []
                j = e

    # ---- pooled tiles: the tiles of MANY pictures, of any sizes, share coding calls; every container keeps its own bytes
    def encode_tiled_items(self, pictures, *args, tile=(512, 512), overlap=0, max_batch=None, pad_to=1, **kwargs) -> List[bytes]:
        """N pictures ``[1, C, H, W]`` of ANY sizes with one C (uint8 in chw or hwc memory, or float32; host or device; mixed within a
        call) -> their N containers, container k byte for byte ``self.encode_tiled(pictures[k], tile=tile, overlap=overlap, pad_to=pad_to)``.  The
        tiles of all pictures are pooled by size (utils.tiling.pool_tiles: the full tiles of every picture share one shape, the edge
        tiles a few more), a chunk of at most ``max_batch`` tiles is cut out of its uint8 pictures by ONE launch
        (nn.kernels.image_tiles_gather; float32 pictures: one copy per tile, and chunks of their own) and coded by one encode() call,
        whose string is split as in encode_items.  ``last_items_calls`` counts the encode() calls.  One encode_tiled per picture when
        a coder cannot split, in training mode, or when the call brings arguments.  With ``pad_to`` the tiles are pooled by their coded
        size and cut with the edges replicated (``pad=True``); ``pad_to=tile`` makes the pool one size."""
        from ...utils import tiling
        self._no_skip_rows(kwargs, "encode_tiled_items")
        pictures = list(pictures)
        for x in pictures:
            self._check_item(x)
            if x.dtype not in (torch.uint8, torch.float32):
                raise TypeError(f"a picture is torch.uint8 or torch.float32, not {x.dtype}")
        if len({x.shape[1] for x in pictures}) > 1:
            raise ValueError("the pictures of one call share their channel count")
        th, tw = self._tile_size(tile)
        grids = [tiling.TileGrid(x.shape[2], x.shape[3], th, tw, overlap=overlap, pad_to=pad_to) for x in pictures]
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        if framing is None:
            out, calls = [], 0
            for x in pictures:
                out.append(self.encode_tiled(x, *args, tile=tile, max_batch=max_batch, overlap=overlap, pad_to=pad_to, **kwargs))
                calls += self.last_items_calls
            self.last_items_calls = calls
            return out
        self.last_items_calls = 0
        pictures = [x if x.device == self.device else x.to(device=self.device) for x in pictures]   # each once, as it lies
        strings = self._encode_pooled(pictures, grids, framing, max_batch)
        return [tiling.pack_tiled(x.shape[1], g.H, g.W, g.th, g.tw, s, overlap=g.overlap, pad_to=g.pad_to)
                for x, g, s in zip(pictures, grids, strings)]

    def decode_tiled_items(self, containers, *args, output_dtype=torch.uint8, layout="chw", max_batch=None, **kwargs) -> List[torch.Tensor]:
        """N containers of encode_tiled / encode_tiled_items, of any picture and tile sizes and overlaps (read from each) -> their N
        pictures, picture k equal to ``self.decode_tiled(containers[k], output_dtype=output_dtype, layout=layout)``.  Tiles of one size
        whose strings' own headers agree (as decode_items keys them) share a decode() call of at most ``max_batch`` tiles, in the
        order of utils.tiling.pool_tiles; ``last_items_calls`` counts the calls.  uint8 results are converted, cropped and pasted by
        ONE launch per call whatever pictures its tiles belong to (nn.kernels.image_tiles_scatter); float32 results by one copy per
        tile.  Overlapped containers: a picture is written by the blend launch of decode_tiled (nn.kernels.image_tiles_blend, one per
        picture) as soon as the last of its tiles is decoded, from views of the pooled batches.  Until then the batches that hold
        its tiles stay resident, and a batch is freed only when every overlapped picture with a tile in it is written: at worst
        4 * C * sh * sw bytes per tile of ALL overlapped pictures of the call, on top of the results.  One decode_tiled per
        container when a coder cannot split, in training mode, or when the call brings arguments.  No ``region=``: decoding a part
        of a picture stays decode_tiled's.  Edge-padded containers (BTL3; ``pad_to`` read from each, and free to differ within a call):
        their tiles are pooled by coded size and cropped to their valid rectangles (the scatter with ``clip=True``)."""
        from ...nn import kernels as K
        self._no_skip_rows(kwargs, "decode_tiled_items")
        from ...utils import tiling
        if "region" in kwargs:
            raise TypeError("decode_tiled_items takes no region: decode a part of a picture with decode_tiled")
        if output_dtype not in (None, torch.float32, torch.uint8):
            raise TypeError(f"output_dtype is torch.float32 or torch.uint8, not {output_dtype}")
        if layout not in K.IMAGE_LAYOUTS:
            raise ValueError(f"layout is 'chw' or 'hwc', not {layout!r}")
        containers = list(containers)
        framing = self._items_framing() if not (args or kwargs or self.training) else None
        if framing is None:
            out, calls = [], 0
            for data in containers:
                out.append(self.decode_tiled(data, *args, output_dtype=output_dtype, layout=layout, max_batch=max_batch, **kwargs))
                calls += self.last_items_calls
            self.last_items_calls = calls
            return out
        heads, steps = zip(*(self._unpack_tiled(data) for data in containers)) if containers else ((), ())
        grids = [tiling.TileGrid(t.H, t.W, t.th, t.tw, t.overlap, t.pad_to) for t in heads]
        as_u8 = output_dtype == torch.uint8
        dtype = torch.uint8 if as_u8 else torch.float32
        self.last_items_calls = self.last_tiles_decoded = 0
        with torch.no_grad(), torch.cuda.device(self.device):
            canvases = []
            for t in heads:
                if layout == "hwc":
                    canvases.append(torch.empty((1, t.H, t.W, t.channels), dtype=dtype, device=self.device).permute(0, 3, 1, 2))
                else:
                    canvases.append(torch.empty((1, t.channels, t.H, t.W), dtype=dtype, device=self.device))
            self._decode_pooled(heads, grids, canvases, framing, max_batch, as_u8, steps=list(steps))
        return canvases

    # ---- tiled pictures under a quantiser step, stated or chosen per picture for a byte budget (INTEGRATION.md "Tiled pictures: step
    # and byte budget").  New entry points: encode_tiled / encode_tiled_items and their containers do not change.
    def _tiled_q_framing(self):
        """The item framing of a stepped tiled call, refusals first: ValueError in training mode and when a coder cannot give every
        image its own body, TypeError when the y coder takes no step."""
        if self.training:
            raise ValueError("tiled coding under a quantiser step is an inference call: the codec is in training mode")
        self._qstep_coder_kwargs(1.0, 1)   # TypeError: not a GaussianConditional y coder
        framing = self._items_framing()
        if framing is None:
            raise ValueError("tiled coding under a quantiser step needs coders that split a batch's string into its images' (split_items)")
        return framing

    def encode_tiled_q(self, image, qstep, tile=(512, 512), max_batch=None, overlap=0, pad_to=1) -> bytes:
        """encode_tiled under a quantiser step of the y latent: ``qstep`` is one step for the picture, or one per tile in grid
        (row-major) order.  -> the BTQ1 container (utils/tiling.py), tile k's string EXACTLY ``self.encode(P_k, qstep=step_k)`` of the
        tile encode_tiled cuts, by encode_tiled's plan: ``last_items_calls`` is the step-less call's."""
        from ...utils import tiling
        self._check_picture(image)
        framing = self._tiled_q_framing()
        _, C, H, W = image.shape
        grid = tiling.TileGrid(H, W, *self._tile_size(tile), overlap=overlap, pad_to=pad_to)
        steps = np.array(np.broadcast_to(check_qsteps(qstep, len(grid)), (len(grid),)), dtype=np.float32)
        out = self._encode_tiles(image, grid, framing, max_batch, steps=steps)
        return tiling.pack_tiled_q(C, H, W, grid.th, grid.tw, out, steps, overlap=grid.overlap, pad_to=grid.pad_to)

    def _check_pictures(self, pictures):
        pictures = list(pictures)
        for x in pictures:
            self._check_picture(x)
        if not pictures:
            raise ValueError("no pictures")
        if len({x.shape[1] for x in pictures}) > 1:
            raise ValueError("the pictures of one call share their channel count")
        return pictures

    def encode_tiled_items_q(self, pictures, qsteps, tile=(512, 512), overlap=0, max_batch=None, pad_to=1) -> List[bytes]:
        """encode_tiled_items under quantiser steps: ``qsteps`` is one step, or one per picture.  -> N BTQ1 containers, container k byte
        for byte ``self.encode_tiled_q(pictures[k], step_k, tile=, overlap=, pad_to=)``, by the pooled plan of encode_tiled_items."""
        from ...utils import tiling
        pictures = self._check_pictures(pictures)
        framing = self._tiled_q_framing()
        th, tw = self._tile_size(tile)
        grids = [tiling.TileGrid(x.shape[2], x.shape[3], th, tw, overlap=overlap, pad_to=pad_to) for x in pictures]
        per_picture = np.broadcast_to(check_qsteps(qsteps, len(pictures)), (len(pictures),))
        steps = [np.full(len(g), s, dtype=np.float32) for g, s in zip(grids, per_picture)]
        self.last_items_calls = 0
        pictures = [x if x.device == self.device else x.to(device=self.device) for x in pictures]
        strings = self._encode_pooled(pictures, grids, framing, max_batch, steps=steps)
        return [tiling.pack_tiled_q(x.shape[1], g.H, g.W, g.th, g.tw, s, q, overlap=g.overlap, pad_to=g.pad_to)
                for x, g, s, q in zip(pictures, grids, strings, steps)]

    def _measure_latents(self, batch):
        """The analysis side of encode()'s module path on one batch: g_a, h_a, the coding of every node before the y node (enqueued,
        not synchronised) and h_s.  -> (the pending bodies of those nodes, y, sigma): what the y coder's encode() was handed, kept on
        the device.  The transforms run here once; the step is chosen and y coded from these tensors."""
        from ...nn import kernels as K
        if batch.dtype == torch.uint8:
            batch = K.image_u8_to_f32(batch)
        node_dict = self._node_generate_process(**self._get_default_node_dict(force_add_default_dynamic_nodes=True))
        latent = self._inference_process({self.DEFAULT_INPUT_NODE_NAME: batch, **node_dict})
        held = {}
        data_dict, _ = self._generative_process(latent, do_encode=True, coder_kwargs={self.QSTEP_NODE: dict(rate_measure=held)})
        nodes = self._coded_nodes()
        return [data_dict[n] for n in nodes if n != self.QSTEP_NODE], held["y"], held["scales"]

    def encode_tiled_items_to_rate(self, pictures, target_bytes=None, target_bpp=None, tile=(512, 512), overlap=0, pad_to=1, max_batch=None,
                                   candidates=16, passes=2, step_range=(2 ** -4, 2 ** 6), return_report=False, workspace_limit=2 << 30):
        """encode_tiled_items_q with ONE step per picture chosen on the GPU so that the picture's whole BTQ1 container -- framing included
        -- fits a byte budget.  Give exactly one target, a number or one per picture: ``target_bytes``, or ``target_bpp`` (budget =
        floor(bpp * H * W / 8), the picture's own H and W).  The host takes utils.tiling.tiled_q_framing_bytes off the budget; the
        rest is the budget of the picture's payload over all its tiles.  Every pooled chunk runs the analysis side once
        (_measure_latents); y and sigma of all chunks stay on the device (``workspace_limit`` bytes at most, else ValueError before
        anything is launched), the candidate steps are rated chunk by chunk into one curve tensor, nn.kernels.rate_steps_groups picks
        the first candidate whose predicted payload fits each picture and refines it ``passes - 1`` times, and every chunk's y is
        coded from the retained tensors under its tiles' steps, read on the device.  -> N containers, container k byte for byte
        ``self.encode_tiled_q(pictures[k], its step)``; with ``return_report`` also a list of per-picture dicts: ``step``,
        ``predicted_bytes``, ``container_bytes``, ``budget``, ``met`` (container <= budget), ``fits``, ``n_tiles`` and per tile
        ``predicted_payload`` and ``payload``.  A picture no candidate fits takes the largest step and reports ``met`` False."""
        from ...nn import kernels as K
        from ...utils import tiling
        from ...utils.rate import NO_FIT, budgets_from, check_passes, first_grid
        pictures = self._check_pictures(pictures)
        framing = self._tiled_q_framing()
        N = len(pictures)
        th, tw = self._tile_size(tile)
        grids = [tiling.TileGrid(x.shape[2], x.shape[3], th, tw, overlap=overlap, pad_to=pad_to) for x in pictures]
        nodes = self._coded_nodes()
        if nodes[-1] != self.QSTEP_NODE:
            raise ValueError(f"a byte budget chooses the step of node '{self.QSTEP_NODE}', which must be the last node coded, not {nodes}")
        ycoder = self.latent_node_entropy_coders[self.QSTEP_NODE]
        lanes = ycoder.stream_lanes
        streams = [getattr(c, "stream_lanes", 1) for c, _ in framing]
        if (target_bytes is None) == (target_bpp is None):
            raise ValueError("give exactly one of target_bytes and target_bpp")
        target = np.asarray(target_bytes if target_bytes is not None else target_bpp, dtype=object).reshape(-1)
        if target.size not in (1, N):
            raise ValueError(f"give one target, or one per picture of the {N} (got {target.size})")
        budgets, framings = np.zeros(N, np.int64), np.zeros(N, np.int64)
        for p, g in enumerate(grids):
            one = target[p if target.size == N else 0]
            budgets[p] = budgets_from(one if target_bytes is not None else None, one if target_bpp is not None else None, 1, g.H, g.W)[0]
            framings[p] = tiling.tiled_q_framing_bytes(g, streams_per_body=streams)
            if budgets[p] <= framings[p]:
                raise ValueError(f"picture {p}: a budget of {budgets[p]} bytes is not above the {framings[p]} bytes of framing its "
                                 f"{len(g)} tiles take (utils.tiling.tiled_q_framing_bytes); nothing is left for the payload")
        grid0 = first_grid(candidates, step_range)
        passes = check_passes(passes)
        # y and sigma of every tile stay resident: 2 * 4 bytes per latent sample, M / 256 samples per coded pixel (6 bytes a pixel at M = 192)
        gen = self.latent_inference_modules
        M = next((int(m.M) for name, m in gen.items() if name.split(self.DEFAULT_EDGE_SPLIT_SYMBOL)[1] == self.QSTEP_NODE and hasattr(m, "M")), 192)
        pixels = sum(g.coded_size(k)[0] * g.coded_size(k)[1] for g in grids for k in range(len(g)))
        curve_means = getattr(ycoder, "rate_curve_means", None)   # the mean-scale coder: the retained sigma is its chunked prior
        need = (12 if curve_means is not None else 8) * M * pixels // 256
        if need > workspace_limit:
            raise ValueError(f"the latents of {sum(len(g) for g in grids)} tiles ({pixels} coded pixels) take {need} bytes on the device, "
                             f"more than workspace_limit={workspace_limit}: code the pictures in several calls")
        self.last_items_calls = 0
        pictures = [x if x.device == self.device else x.to(device=self.device) for x in pictures]
        with torch.no_grad(), torch.cuda.device(self.device):
            chunks, latents, extras, tile_of = [], [], [], {}
            for refs, batch in self._pooled_batches(pictures, grids, max_batch):
                self.last_items_calls += 1
                before, y, scales = self._measure_latents(batch)
                words = torch.zeros((len(refs),), device=y.device, dtype=torch.int32)
                for body in before:   # the words an image has spent on its earlier streams: on the device, as the coder counted them
                    if not hasattr(body, "_handle") or body._handle is None:
                        raise ValueError("a byte budget needs the earlier nodes' coders to enqueue their streams (encode(lazy=True))")
                    words += body._handle["nwords"].clamp(min=0).reshape(len(refs), -1).sum(1, dtype=torch.int32)
                for ref in refs:
                    tile_of[(ref.picture, ref.index)] = len(tile_of)
                chunks.append((refs, before))
                latents.append((y, scales))
                extras.append(words)
            groups = [[tile_of[(p, k)] for k in range(len(g))] for p, g in enumerate(grids)]
            payload_budgets = torch.from_numpy(budgets - framings).to(self.device)
            steps, choice, pred, tile_steps, tile_pred = K.rate_steps_groups(
                latents, groups, payload_budgets, torch.cat(extras), grid0, passes, ycoder._scale_table_dev, ycoder._tables,
                ycoder.scale_bound, lanes, means=curve_means)
            strings = [[None] * len(g) for g in grids]
            spent = [[0] * len(g) for g in grids]

            def finish(refs, before, ybody):   # the one synchronisation of a chunk: its bytes, framed and split per tile
                merged = merge_bodies(before + [ybody])
                spent_words = self._words_coded(dict(zip(nodes, before)), nodes[:-1], len(refs))
                for j, ((p, k, _, _), one) in enumerate(zip(refs, self._split_string(merged, len(refs), framing))):
                    strings[p][k], spent[p][k] = one, int(spent_words[j])

            row, waiting = 0, None
            for c, (refs, before) in enumerate(chunks):
                y, scales = latents[c]
                latents[c] = None   # coded from here on: the chunk's latents go when its symbols are written
                ybody = ycoder._encode_q(y, scales, tile_steps[row:row + len(refs)], lazy=True, steps_on_device=True)
                row += len(refs)
                if waiting is not None:   # the chunk before is framed on the host while this one is coded
                    finish(*waiting)
                waiting = (refs, before, ybody)
            host = [t.cpu().numpy() for t in (steps, choice, pred, tile_pred, torch.cat(extras))]   # after the last chunk's coding is enqueued
            finish(*waiting)
        steps, choice, pred, tile_pred, extra = host
        for p, g in enumerate(grids):
            for k in range(len(g)):
                if spent[p][k] != int(extra[tile_of[(p, k)]]):
                    raise RuntimeError(f"picture {p}, tile {k}: an earlier stream was re-coded with a larger buffer after the step was chosen; "
                                       "its length is not the one the budget was charged")
        out = [tiling.pack_tiled_q(x.shape[1], g.H, g.W, g.th, g.tw, s, float(q), overlap=g.overlap, pad_to=g.pad_to)
               for x, g, s, q in zip(pictures, grids, strings, steps)]
        if not return_report:
            return out
        report = []
        for p, g in enumerate(grids):
            mine = [tile_of[(p, k)] for k in range(len(g))]
            report.append(dict(step=float(steps[p]), predicted_bytes=int(pred[p] + framings[p]), container_bytes=len(out[p]),
                               budget=int(budgets[p]), met=len(out[p]) <= int(budgets[p]), fits=not (int(choice[p]) & NO_FIT), n_tiles=len(g),
                               predicted_payload=tile_pred[mine].astype(np.int64),
                               payload=np.array([int(self.payload_bytes(s, 1)[0]) for s in strings[p]], dtype=np.int64)))
        return out, report

    def encode_tiled_to_rate(self, image, target_bytes=None, target_bpp=None, tile=(512, 512), overlap=0, pad_to=1, max_batch=None,
                             candidates=16, passes=2, step_range=(2 ** -4, 2 ** 6), return_report=False, workspace_limit=2 << 30):
        """One picture coded as tiles into a byte budget that covers its whole BTQ1 container: encode_tiled_items_to_rate of the one
        picture.  -> the container, byte for byte ``self.encode_tiled_q(image, the chosen step)``; with ``return_report`` also its
        report (a dict)."""
        self._check_picture(image)
        out = self.encode_tiled_items_to_rate([image], target_bytes=target_bytes, target_bpp=target_bpp, tile=tile, overlap=overlap,
                                              pad_to=pad_to, max_batch=max_batch, candidates=candidates, passes=passes,
                                              step_range=step_range, return_report=return_report, workspace_limit=workspace_limit)
        return (out[0][0], out[1][0]) if return_report else out[0]

    def forward(self, data, *args, **kwargs):
        """Eval-mode forward: quantised reconstruction without entropy coding (latent_graph.py:870-1230
        minus the training losses)."""
        with torch.no_grad():
            node_dict = self._node_generate_process(**self._get_default_node_dict(force_add_default_dynamic_nodes=True, **kwargs))
            latent = self._inference_process({self.DEFAULT_INPUT_NODE_NAME: data.to(self.device), **node_dict})
            # the coders' forward() inside encode() skips the likelihood pass (nobody reads it there); here it is the
            # point of the call (prior_entropy / estimated_bpd), as in the reference's forward
            coders = [c for c in self.latent_node_entropy_coders.values() if hasattr(c, "estimate_rate")]
            saved = [c.estimate_rate for c in coders]
            for c in coders:
                c.estimate_rate = True
            try:
                data_dict, prior_dict = self._generative_process(latent)
            finally:
                for c, v in zip(coders, saved):
                    c.estimate_rate = v
            # rate metrics (latent_graph.py:1168-1178): nats per image summed over the coded nodes, bits per dimension
            total_prior_entropy, estimated_bpd = 0, 0
            for name, module in self.latent_node_entropy_coders.items():
                pe = module.get_raw_cache("metric_dict").get("prior_entropy") if hasattr(module, "get_raw_cache") else None
                if pe is not None:
                    total_prior_entropy = total_prior_entropy + pe
                    estimated_bpd = estimated_bpd + pe / math.log(2) / (data.numel() / data.size(0))
            self.update_cache("metric_dict", prior_entropy=total_prior_entropy, estimated_bpd=estimated_bpd)
            return data_dict[self.DEFAULT_INPUT_NODE_NAME]

    def update_state(self, *args, **kwargs) -> None:  # latent_graph.py:1297-1301
        for coder in self.latent_node_entropy_coders.values():
            coder.update_state(*args, **kwargs)

    # ---- VariableRate / Complexity / Task (latent_graph.py:1660-1691)
    def set_rate_level(self, level, *args, **kwargs) -> None:
        assert 0 <= level < max(1, self._num_rate_levels)
        self._current_rate_level = level

    @property
    def num_rate_levels(self):
        return max(1, self._num_rate_levels)

    def set_complex_level(self, level, *args, **kwargs) -> None:
        assert 0 <= level < max(1, self._num_complex_levels)
        self._current_complex_level = level

    @property
    def num_complex_levels(self):
        return max(1, self._num_complex_levels)

    def set_complexity_level_params(self, params_per_level: List[Dict[str, Any]]):
        """Install a ready-made outcome of the search (latent_graph.py:1615-1619): one dict of controller-node values
        (e.g. slim one-hots pgmxy/pgmyz/pgmzy/pgmyx) per level."""
        dev = self.device
        self._complexity_param_all_levels = nn.ModuleList([ParamDictModuleWrapper(p) for p in params_per_level]).to(dev)
        self._num_complex_levels = len(params_per_level)
        self.complexity_level_greedy_search = True
        if not hasattr(self, "_complexity_param_valid"):
            self.register_buffer("_complexity_param_valid", torch.tensor([True], device=dev))
        self._complexity_param_valid.fill_(True)
        self._valid_host = None
        if len(self.complexity_metric_list) > 0:
            self.register_buffer("_complexity_metric_list_cache",
                                 torch.zeros(self._num_complex_levels, len(self.complexity_metric_list), device=dev))

    def get_current_complex_metrics(self, *args, **kwargs):  # latent_graph.py:1675-1687
        if not hasattr(self, "_complexity_metric_list_cache"):
            return dict()
        row = self._complexity_metric_list_cache[self._current_complex_level]
        return {name: row[i].item() for i, name in enumerate(self.complexity_metric_list)}

    # ---- complexity accounting and the greedy level search (latent_graph.py:1303-1640)
    def get_current_flops(self, input=None):
        """Sum of the dynamic transforms' operation counters of the last forward (nn/base.py:675-680)."""
        total = 0.0
        for m in self.modules():
            if m is not self and hasattr(m, "get_current_flops"):
                total += float(m.get_current_flops())
        return total

    def _test_dataset_complexity_performance(self, dataset, *args, performance_method="loss", complexity_method="FLOPs",
                                             loss_mode=None, **node_params):
        """(complexity, performance) of one controller setting over a dataset, both divided by the number of input
        elements (latent_graph.py:1320-1395).

        performance "loss" = the rate and distortion loss terms: loss_rate = prior_entropy / ln 2 of every coded node
        (bits per image; compressai_coder.py:213-215, pgm_coder.py:516) + loss_distortion = lambda_rd * SSE per image
        (:83-88).  The reference evaluates them in train mode, i.e. with its additive-uniform-noise proxies, so its
        number is a random variable (loss_mode "train": every coder's forward adds U(-.5, .5) instead of rounding --
        torch_ans.py:127-136 and upstream quantize(..., "noise") -- drawn from torch's CUDA generator); the default
        (loss_mode "eval", or complexity_level_greedy_search_loss_mode) evaluates them on the ROUNDED latents the codec
        actually codes, which is deterministic.  complexity "FLOPs" = get_current_flops(); the timing variants
        ("compress_time", "decompress_time", "total_time") wall-clock encode / decode."""
        if performance_method != "loss":
            raise NotImplementedError(performance_method)
        coders = [c for c in self.latent_node_entropy_coders.values() if hasattr(c, "estimate_rate")]
        saved = [c.estimate_rate for c in coders]
        for c in coders:
            c.estimate_rate = True
        loss_mode = loss_mode or self.complexity_level_greedy_search_loss_mode
        proxied = [m for c in self.latent_node_entropy_coders.values() if isinstance(c, nn.Module) for m in c.modules()]
        for m in proxied:
            m.rate_proxy = "noise" if loss_mode == "train" else "round"
        performance, complexity, total_dims = 0.0, 0.0, 0
        searching, self._searching = self._searching, True
        try:
            for data in dataset:
                if isinstance(data, (list, tuple)):
                    data = data[0]
                total_dims += data.numel()
                self.forward(data, *args, **node_params)
                loss = 0.0
                for name, coder in self.latent_node_entropy_coders.items():
                    md = coder.get_raw_cache("metric_dict") if hasattr(coder, "get_raw_cache") else {}
                    if "prior_entropy" in md:
                        loss += float(md["prior_entropy"]) / math.log(2)
                    if "weighted_distortion" in md:
                        loss += float(md["weighted_distortion"])
                performance += loss
                if complexity_method == "FLOPs":
                    complexity += self.get_current_flops()
                elif complexity_method in ("compress_time", "decompress_time", "total_time"):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    byte_string = self.encode(data, *args, **node_params)
                    t1 = time.time()
                    out = self.decode(byte_string, *args, **node_params)
                    if isinstance(out, torch.Tensor) and out.is_cuda:
                        torch.cuda.synchronize()
                    t2 = time.time()
                    complexity += {"compress_time": t1 - t0, "decompress_time": t2 - t1, "total_time": t2 - t0}[complexity_method]
                else:
                    raise NotImplementedError(complexity_method)
                self.reset_all_cache()
        finally:
            self._searching = searching
            for m in proxied:
                m.rate_proxy = "round"
            for c, v in zip(coders, saved):
                c.estimate_rate = v
        if total_dims == 0:
            raise ValueError("complexity_level_greedy_search_dataset is empty")
        return complexity / total_dims, performance / total_dims

    def post_training_process(self, *args, force=False, dataset=None, **kwargs) -> None:
        """latent_graph.py:1397-1640: fill the complexity levels by searching the controller settings.  Runs once
        (``_complexity_param_valid``) unless ``force``; ``dataset`` overrides complexity_level_greedy_search_dataset."""
        if not self.complexity_level_greedy_search:
            return
        self.update_state()
        if not (force or not self._levels_valid()):
            return
        names = list(self.complexity_level_controller_nodes)
        if self.complexity_level_greedy_search_custom_params is not None:
            levels = [dict(idx) for idx in self.complexity_level_greedy_search_custom_params]
            rows = None
        else:
            if self.complexity_level_greedy_search_iterative:
                raise NotImplementedError("complexity_level_greedy_search_iterative (see complexity_search.py)")
            data = dataset if dataset is not None else self.complexity_level_greedy_search_dataset
            if data is None:
                raise ValueError("complexity_level_greedy_search_dataset is required for the complexity search")
            if self.complexity_level_greedy_search_dataset_cached or not isinstance(data, (list, tuple)):
                data = list(data)
            gens = {n: self.node_generators[n] for n in names}

            def evaluate(idx):
                return self._test_dataset_complexity_performance(
                    data, performance_method=self.complexity_level_greedy_search_performance_metric,
                    complexity_method=self.complexity_level_greedy_search_complexity_metric,
                    **{n: gens[n](idx[n]) for n in names})

            result = search_complexity_levels(
                evaluate, names, {n: gens[n].min_sample for n in names}, {n: gens[n].max_sample for n in names},
                num_levels=self._num_complex_levels, custom_constraint=self.complexity_level_greedy_search_custom_constraint)
            levels = result.levels
            rows = result.metric_rows(self.complexity_metric_list, self.complexity_level_greedy_search_complexity_metric,
                                      self.complexity_level_greedy_search_performance_metric)
            self.complexity_search_result = result
        dev = self.device
        self._complexity_param_all_levels = nn.ModuleList(
            [ParamDictModuleWrapper({n: self.node_generators[n](v) for n, v in lvl.items()}) for lvl in levels]).to(dev)
        self._num_complex_levels = len(levels)
        if rows is not None and hasattr(self, "_complexity_metric_list_cache"):
            self._complexity_metric_list_cache = torch.tensor(rows, dtype=torch.float32, device=dev)
        self._complexity_param_valid.fill_(True)
        self._valid_host = None
        self.eval()

    def set_task(self, task, *args, **kwargs) -> bool:
        if self._num_tasks == 0:
            return False
        self._current_task_idx = self.task_names.index(task) if task in self.task_names else int(task)
        return True

    @property
    def num_tasks(self):
        return max(1, self._num_tasks)
