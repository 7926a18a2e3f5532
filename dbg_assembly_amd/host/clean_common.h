// clean_common.h -- what bin/clean_adapter and bin/clean_lowqual share on top of cli_common.h: the FASTQ record loop of the
// reference (clean_illumina/clean_adapter.cpp:376-387, the same in clean_lowqual.cpp) and a batch of records on its way to the
// device (CLEAN section of include/dbgk.h).
#pragma once
#include <unistd.h>
#include <cstdio>
#include <ctime>

#include "cli_common.h"

static const uint64_t BatchReads = 1 << 20;   // records per device batch
static const uint64_t BatchBases = 256 << 20; // ... or this many bases, whichever comes first

// a batch of records: heads, reads and qualities as read, and the reads (for clean_lowqual the qualities too) back to back
struct RecordBatch {
	vector<string> heads, reads, quals;
	uint64_t bases = 0;
	size_t size() const { return heads.size(); }
	bool full() const { return size() >= BatchReads || bases >= BatchBases; }
	void clear()
	{
		heads.clear(); reads.clear(); quals.clear();
		bases = 0;
	}
	// the record loop: a line that starts with '@' opens a record and the next three lines are read, separator and quality
	// whatever they hold; every other line outside a record is skipped.  false at the end of the file.
	bool fill(LineReader &in, uint64_t &total_raw_reads, uint64_t &total_raw_bases)
	{
		string head, read, unused, qual;
		while (!full() && in.getline(head)) {
			if (head.empty() || head[0] != '@') continue;
			in.getline(read);
			in.getline(unused);
			in.getline(qual);
			total_raw_reads++;
			total_raw_bases += read.size();
			bases += read.size();
			heads.push_back(head);
			reads.push_back(read);
			quals.push_back(qual);
		}
		return full();
	}
	// every record as four lines, also when read and quality were emptied
	void write(GzWriter &out) const
	{
		string text;
		for (size_t i = 0; i < size(); i++) {
			text += heads[i]; text += '\n';
			text += reads[i]; text += "\n+\n";
			text += quals[i]; text += '\n';
			if (text.size() >= (64u << 20)) {
				out.write(text);
				text.clear();
			}
		}
		out.write(text);
	}
};
