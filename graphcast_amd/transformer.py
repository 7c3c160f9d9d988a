"""``weathernext1_gen/transformer.py::MeshTransformer`` on the device: GenCast's processor on a ``TypedGraph``.

The reference wraps ``sparse_transformer.Transformer`` so that it takes the mesh-node features of a typed graph in
[nodes, batch, ...] order: the adjacency comes from the graph's ``mesh`` edge set (rows = senders, plus self edges,
built on the first call), the features are transposed to [batch, nodes, ...] and back.  Same here, on
``graphcast_amd.sparse_transformer.Transformer``; parameters are the haiku tree under
``<name>/~/transformer/...`` (``hk.name_like('__init__')`` scopes the inner module in the wrapper's constructor).
"""
from typing import Any, Mapping, Optional

import numpy as np
import torch

from graphcast_amd import sparse_transformer
from graphcast_amd import typed_graph


def _get_adj_matrix_for_edge_set(graph: typed_graph.TypedGraph, edge_set_name: str, add_self_edges: bool):
  """The graph's edge set as a boolean csr [senders, receivers] (+ self edges) (reference transformer.py:32-55)."""
  key = graph.edge_key_by_name(edge_set_name)
  snd_set, rcv_set = key.node_sets
  n_s, n_r = int(np.asarray(graph.nodes[snd_set].n_node)[0]), int(np.asarray(graph.nodes[rcv_set].n_node)[0])
  s, r = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, np.int64) for a in graph.edges[key].indices)
  if add_self_edges:
    assert snd_set == rcv_set
  from scipy import sparse
  adj = sparse.csr_matrix((np.ones(len(s), np.bool_), (s, r)), shape=(n_s, n_r))
  if add_self_edges:
    adj = adj + sparse.identity(n_s, dtype=np.bool_, format="csr")
  return sparse.csr_matrix(adj, dtype=np.bool_)


class MeshTransformer:
  """A Transformer for inputs with ordering [nodes, batch, ...] (reference transformer.py:58-133).

  ``transformer_ctor`` defaults to ``sparse_transformer.Transformer``; ``transformer_kwargs`` are its arguments
  (``attention_k_hop``, ``attention_type``, ``num_layers``, ...).  ``params``, ``device``, ``precision`` and
  ``node_positions`` are handed to it."""

  def __init__(self, transformer_ctor=None, transformer_kwargs: Mapping[str, Any] = None,
               name: Optional[str] = None, *, params: Mapping = None, device="cuda:0",
               precision: Optional[str] = None, node_positions=None):
    self.name = name or "mesh_transformer"
    self._ctor = transformer_ctor or sparse_transformer.Transformer
    self._kwargs = dict(transformer_kwargs or {})
    self._extra = dict(params=params, device=device, precision=precision, node_positions=node_positions)
    self._batch_first_transformer = None

  def _maybe_init_batch_first_transformer(self, x: typed_graph.TypedGraph):
    if self._batch_first_transformer is None:
      self._batch_first_transformer = self._ctor(
          adj_mat=_get_adj_matrix_for_edge_set(x, "mesh", add_self_edges=True), **self._kwargs, **self._extra)

  def __call__(self, x: typed_graph.TypedGraph, global_norm_conditioning: torch.Tensor) -> typed_graph.TypedGraph:
    if set(x.nodes.keys()) != {"mesh_nodes"}:
      raise ValueError(f"Expected x.nodes to have key `mesh_nodes`, got {x.nodes.keys()}.")
    features = x.nodes["mesh_nodes"].features
    if features.dim() != 3:
      raise ValueError(f'Expected `x.nodes["mesh_nodes"].features` to be 3, got {features.dim()}.')
    self._maybe_init_batch_first_transformer(x)
    y = features.transpose(0, 1).contiguous()
    y = self._batch_first_transformer(y, global_norm_conditioning)
    y = y.transpose(0, 1).contiguous()
    return x._replace(nodes={"mesh_nodes": x.nodes["mesh_nodes"]._replace(features=y.to(features.dtype))})
