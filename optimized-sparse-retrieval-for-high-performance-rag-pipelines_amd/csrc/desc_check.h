// desc_check.h -- the check of an srx_index_desc that the entry points working straight from a descriptor share: srx_score_docs
// (score_docs.hip, which defines it) and srx_filter_from_terms (terms.hip).  A host function with hidden visibility, not part of
// the C ABI; every message starts with the caller's name `who`.
#pragma once
#include "srx_common.h"

int srx_check_index_desc(const char *who, const srx_index_desc *d);
