"""Mirror of bindings/python/flashlight/lib/text/decoder/__init__.py:12-32."""
from text_amd.flashlight_lib_text_decoder import (  # noqa: F401
    CriterionType, DecodeResult, KenLM, LexiconDecoder, LexiconDecoderOptions, LexiconFreeDecoder,
    LexiconFreeDecoderOptions, LM, LMState, SmearingMode, Trie, TrieNode, ZeroLM)
from ._seq2seq import (  # noqa: F401,E402
    EmittingModelState, LexiconFreeSeq2SeqDecoder, LexiconFreeSeq2SeqDecoderOptions, LexiconSeq2SeqDecoder,
    LexiconSeq2SeqDecoderOptions, create_emitting_model_state,
    get_obj_from_emitting_model_state)
