from .proposal_target_layer import ProposalTargetLayer

__all__ = {'ProposalTargetLayer': ProposalTargetLayer}
