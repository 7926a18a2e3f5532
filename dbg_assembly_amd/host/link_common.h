// link_common.h -- what bin/link_scaffold, bin/link_contig and bin/link_supertig share on top of cli_common.h: the option variables
// all three have, the reference's contig file format (link_scaffold/link_func.cpp:99-136) with the checks on the contig names, the
// checked part of one 2ctg line, display_data_in_link, the reports on stderr they all write, the two-call emit and the
// repeat-contig files.  The handle differs (dbgk_link, dbgk_fill or dbgk_super: LINK, FILL and SUPER sections of include/dbgk.h),
// so the C calls come in as callables.
#pragma once
#include <unistd.h>
#include <cstdio>
#include <ctime>

#include "cli_common.h"

static string Output_prefix = "Output";
static int PairNumCut = 3;

static const size_t BatchRecords = 1 << 22; // records per device batch

// read_contig_file (link_func.cpp:99-136) without the empty strings of the even nodes: contig c is node 2c + 1
static void read_contig_file(const string &file, vector<string> &seqs, vector<string> &ids)
{
	ifstream infile(file.c_str());
	if (!infile) cerr << "fail to open input file " << file << endl;
	string contig_str, line;
	while (getline(infile, line, '\n')) {
		if (!line.empty() && line[0] == '>') {
			vector<string> vec_head;
			split(line, vec_head, "> \t");
			ids.push_back(vec_head.empty() ? string() : vec_head[0]);
			if (contig_str.size() > 0) seqs.push_back(contig_str);
			contig_str.clear();
		} else {
			contig_str += line;
		}
	}
	if (contig_str.size() > 0) seqs.push_back(contig_str);
}

// ctgStr2Id (link_func.h:130)
static int ctgStr2Id(const string &s) { return s.size() > 4 ? atoi(s.c_str() + 4) : 0; }

// the contig file as the three programs take it in, or exit(1)
static void load_contigs(const char *prog, const string &file, vector<string> &ids, vector<string> &seqs, vector<uint32_t> &lens, uint64_t &total_len)
{
	read_contig_file(file, seqs, ids);
	const size_t n_contigs = seqs.size();
	lens.resize(n_contigs);
	total_len = 0;
	for (size_t i = 0; i < n_contigs; i++) {
		if (seqs[i].size() >= (1ull << 31)) {
			cerr << prog << ": contig " << ids[i] << " is longer than 2^31 - 1 bases" << endl;
			exit(1);
		}
		lens[i] = (uint32_t)seqs[i].size();
		total_len += seqs[i].size();
	}
	// the reference finds a contig's node through the number in its name: anything but 2c + 1 for contig c is undefined there
	if (ids.size() != n_contigs) {
		cerr << prog << ": " << file << " has a record without sequence" << endl;
		exit(1);
	}
	for (size_t i = 0; i < n_contigs; i++)
		if (ctgStr2Id(ids[i]) < 0 || (size_t)ctgStr2Id(ids[i]) != 2 * i + 1) {
			cerr << prog << ": contig " << i + 1 << " of " << file << " is named " << ids[i] << ", its number must be " << 2 * i + 1
			     << " (the contig stage and " << prog << " number contigs 1, 3, 5, ...)" << endl;
			exit(1);
		}
	cerr << "\nInput contig number: " << n_contigs << endl;
	cerr << "Input contig length: " << total_len << endl;
	cerr << "Read contigs into memory finished !" << endl;
}

// one line of a 2ctg file split into v: false for a '#' line and for an empty one; otherwise 19 fields or more (the reference reads
// vec_line[18] whatever the line holds) with the nodes id1 and id2 of two contigs of the contig file, or exit(1)
static bool split_map_line(const char *prog, const string &file, const string &line, size_t n_contigs, vector<string> &v, int &id1, int &id2)
{
	if (!line.empty() && line[0] == '#') return false;
	v.clear();
	split(line, v, " \t\n");
	if (v.size() < 19) {
		if (v.empty()) return false;
		cerr << prog << ": a line of " << file << " has " << v.size() << " fields, 19 are needed" << endl;
		exit(1);
	}
	id1 = ctgStr2Id(v[4]);
	id2 = ctgStr2Id(v[14]);
	if (id1 % 2 != 1 || id2 % 2 != 1 || id1 < 1 || id2 < 1 || (size_t)(id1 / 2) >= n_contigs || (size_t)(id2 / 2) >= n_contigs) {
		cerr << prog << ": " << v[4] << " / " << v[14] << " in " << file << " is no contig of the contig file" << endl;
		exit(1);
	}
	return true;
}

static void report_link_classes(const dbgk_link_counters &ctr)
{
	cerr << "\nFR_link_num: " << ctr.fr << endl;
	cerr << "RF_link_num: " << ctr.rf << endl;
	cerr << "FF_link_num: " << ctr.ff << endl;
	cerr << "RR_link_num: " << ctr.rr << endl;
	cerr << "Effect_link_num: " << ctr.fr + ctr.rf + ctr.ff + ctr.rr << endl;
	cerr << "Wrong_link_num: " << ctr.wrong << endl;
}

// snapshot(stage, inlink, link, entries) is dbgk_link_snapshot, dbgk_fill_snapshot or dbgk_super_snapshot on the program's handle,
// die() included
template <class Snapshot>
static void report_3prime_links(Snapshot snapshot, size_t n_nodes)
{
	vector<uint8_t> link(n_nodes);
	snapshot(0, nullptr, link.data(), nullptr);
	uint64_t total_link_num = 0, uniq_link_num = 0, multiple_link_num = 0, empty_link_num = 0;
	for (size_t i = 1; i < n_nodes; i += 2) {
		if (link[i] == 0) empty_link_num++;
		else if (link[i] == 1) uniq_link_num++;
		else multiple_link_num++;
		total_link_num++;
	}
	cerr << "Number and ratio of contigs having a unique 3'-link: " << uniq_link_num << "  " << (float)uniq_link_num / total_link_num << endl;
	cerr << "Number and ratio of contigs having multiple 3'-link: " << multiple_link_num << "  " << (float)multiple_link_num / total_link_num << endl;
	cerr << "Number and ratio of contigs having zero 3'-link:     " << empty_link_num << "  " << (float)empty_link_num / total_link_num << endl;
}

// display_data_in_link (link_func.cpp:515-537)
template <class Snapshot>
static void display_data_in_link(Snapshot snapshot, int stage, const vector<uint64_t> &first, const string &file)
{
	const size_t n_nodes = first.size() - 1;
	vector<uint8_t> inlink(n_nodes), link(n_nodes);
	vector<dbgk_link_entry> e(first[n_nodes] + 1);
	snapshot(stage, inlink.data(), link.data(), e.data());
	FILE *out = fopen(file.c_str(), "w");
	if (!out) {
		cerr << "fail to open file" << file << endl;
		return;
	}
	fputs("ctg_id\tincoming_link_num\toutgoing_link_num\tlinked_id,pair_num,sum_size,avg_size;\n", out);
	for (size_t i = 1; i < n_nodes; i++) {
		fprintf(out, "%zu\t%d\t%d", i, (int)inlink[i], (int)link[i]);
		for (uint64_t j = first[i]; j < first[i + 1]; j++)
			if (e[j].freq > 0)
				fprintf(out, "\t%u,%u,%lld,%lld", e[j].target, e[j].freq, (long long)e[j].size, (long long)(e[j].size / (int64_t)e[j].freq));
		fputc('\n', out);
	}
	fclose(out);
}

// the sequences of all scaffolds from one device call: emit(out, capacity, out_len) is dbgk_link_emit, dbgk_fill_emit or
// dbgk_super_emit (`what`) on the program's contigs and items, called once for the size and once for the bytes
template <class Emit>
static string emit_sequences(Emit emit, const char *what)
{
	uint64_t seq_len = 0;
	int rc = emit(nullptr, 0, &seq_len);
	if (rc && rc != DBGK_ERR_CAPACITY) die(what, rc);
	string seq(seq_len, '\0');
	if (seq_len && (rc = emit(&seq[0], seq_len, &seq_len))) die(what, rc);
	return seq;
}

struct ContigTally {
	uint64_t num = 0, len = 0;
};

// the repeat contigs as scaffolds of their own, <stem>.seq.fa and <stem>.pos.tab, numbered on from id under the program's tag
static ContigTally write_repeat_contigs(const string &stem, const char *tag, int id, const vector<int32_t> &repeats, uint64_t n_repeats,
                                        const vector<string> &ids, const vector<string> &seqs, const vector<uint32_t> &lens)
{
	ofstream SingletFile((stem + ".seq.fa").c_str());
	if (!SingletFile) cerr << "fail to open file" << stem + ".seq.fa" << endl;
	ofstream SingletPosFile((stem + ".pos.tab").c_str());
	if (!SingletPosFile) cerr << "fail to open file" << stem + ".pos.tab" << endl;
	ContigTally excluded;
	for (uint64_t r = 0; r < n_repeats; r++) {
		const int32_t ctg = repeats[r];
		const uint64_t len = lens[ctg];
		id += 2;
		SingletFile << ">" << tag << id << "   fragment_num:1   length:" << len << "   lenwogap:" << len << "   RepeatNode\n" << seqs[ctg] << "\n";
		SingletPosFile << ">" << tag << id << "\n\t" << ids[ctg] << "\t1\t" << len << "\t" << len << "\tF\n";
		excluded.num++;
		excluded.len += len;
	}
	return excluded;
}

static void report_contig_use(ContigTally included, ContigTally excluded, uint64_t total_num, uint64_t total_len)
{
	cerr << "\nIncluded contig number: " << included.num << "  " << (float)included.num / total_num << endl;
	cerr << "Included contig length: " << included.len << "  " << (float)included.len / total_len << endl;
	cerr << "Excluded repeat contig number: " << excluded.num << "  " << (float)excluded.num / total_num << endl;
	cerr << "Excluded repeat contig length: " << excluded.len << "  " << (float)excluded.len / total_len << endl;
}
